"""GPU parity tests: the HIP megakernel (through the C ABI) against the CPU oracle on the
same seeded inputs.  Tolerance: north_star's per-pixel RMSE <= 1e-3 on the normalised
image; the arithmetic contract makes the paths identical, so the observed
error is ~1e-8 and the tests also assert a much tighter bound and equal ray counts."""
import numpy as np
import pytest

from common import M, O, hostsim_bvh, hostsim_render, oracle_scene, rmse, tree_containment_errors

pytestmark = pytest.mark.gpu

RMSE_TOL = 1e-3        # BASELINE.json north_star
RMSE_TIGHT = 2e-6      # what the arithmetic contract actually delivers (float association only)
DRAIN_DEFAULT = 64     # option drain_below as moptix_create leaves it (csrc/api_context.h Options::drainBelow)

CASES = [
    ("spheres", dict(farg=0.5), (160, 90), 4),
    ("spheres", dict(farg=0.0), (160, 90), 2),
    ("cornell_quads", {}, (64, 64), 4),
    ("random_spheres", dict(iarg=97), (96, 54), 2),
    ("random_spheres", dict(iarg=497), (64, 36), 1),
    ("file:coffee", {}, (96, 54), 2),
    ("file:coffee", {}, (200, 112), 3),
]


@pytest.mark.parametrize("kind,kw,res,spp", CASES)
def test_render_matches_oracle(gpu_ctx, kind, kw, res, spp):
    hs = M.HostScene(kind, res[0], res[1], **kw)
    seeds = M.launch_seeds(spp)
    gpu_ctx.load(hs)
    gpu_ctx.accum_clear()
    st = gpu_ctx.render_counted(seeds)
    g = gpu_ctx.accum_read()
    o, ost = oracle_scene(hs).render(seeds)
    e = rmse(g / spp, o / spp)
    assert e <= RMSE_TOL
    assert e <= RMSE_TIGHT, "paths diverged: rmse %g" % e
    assert (st.primaryRays, st.bounceRays, st.shadowRays) == (ost.primaryRays, ost.bounceRays, ost.shadowRays)
    assert st.closestHits == ost.closestHits
    # the timed (non-counting) kernel must give the same bits as the counting one
    gpu_ctx.accum_clear()
    gpu_ctx.render(seeds)
    assert np.array_equal(gpu_ctx.accum_read(), g)


@pytest.mark.parametrize("variant", [0, 3, 4])
def test_all_kernel_variants_are_bit_identical(gpu_ctx, variant):
    """The three schedulers (per-lane, workgroup-shared slot queues, and the per-bounce packets of pt_packet.h on the
    shared queues) run the same per-path arithmetic: identical images, identical ray counts, and parity with the oracle."""
    hs = M.HostScene("file:coffee", 200, 112)
    seeds = M.launch_seeds(3)
    default = gpu_ctx.get_option("kernel_variant")
    try:
        gpu_ctx.set_option("kernel_variant", variant)
        gpu_ctx.load(hs)
        gpu_ctx.accum_clear()
        st = gpu_ctx.render_counted(seeds)
        g = gpu_ctx.accum_read()
        gpu_ctx.accum_clear()
        gpu_ctx.render(seeds)
        g2 = gpu_ctx.accum_read()
    finally:
        gpu_ctx.set_option("kernel_variant", default)
    o, ost = oracle_scene(hs).render(seeds)
    assert np.array_equal(g, g2)
    assert rmse(g / 3, o / 3) <= RMSE_TIGHT
    assert st.rays == ost.rays and st.closestHits == ost.closestHits
    gpu_ctx.set_option("kernel_variant", 0)
    gpu_ctx.load(hs); gpu_ctx.accum_clear(); gpu_ctx.render(seeds)
    ref = gpu_ctx.accum_read()
    gpu_ctx.set_option("kernel_variant", default)
    assert np.array_equal(g, ref)


def test_render_in_passes_equals_single_pass(gpu_ctx):
    """A batch that does not fit the per-sample buffer is cut into passes of whole launches;
    the ordered reduction keeps the result bit-identical."""
    hs = M.HostScene("spheres", 160, 90, farg=0.5)
    seeds = M.launch_seeds(7)
    gpu_ctx.load(hs)
    gpu_ctx.accum_clear(); gpu_ctx.render(seeds); a = gpu_ctx.accum_read()
    mb = gpu_ctx.get_option("sample_buffer_mb")
    try:
        gpu_ctx.set_option("sample_buffer_mb", 1)     # 160x90x12 B = 0.17 MB per launch -> 5+2
        gpu_ctx.accum_clear(); gpu_ctx.render(seeds); b = gpu_ctx.accum_read()
    finally:
        gpu_ctx.set_option("sample_buffer_mb", mb)
    assert np.array_equal(a, b)


def test_launch_by_launch_equals_fused(gpu_ctx):
    """nSeeds moptix_launch calls (MinimalOptiX.cpp:544-546) == one fused moptix_render."""
    hs = M.HostScene("spheres", 96, 54, farg=0.5)
    seeds = M.launch_seeds(5)
    gpu_ctx.load(hs)
    gpu_ctx.accum_clear()
    for s in seeds:
        gpu_ctx.launch(int(s))
    a = gpu_ctx.accum_read()
    gpu_ctx.accum_clear()
    gpu_ctx.render(seeds)
    b = gpu_ctx.accum_read()
    assert np.array_equal(a, b)


@pytest.mark.parametrize("builder", [1, 0])
@pytest.mark.parametrize("leaf", [1, 4, 8])
def test_device_lbvh_equals_host_mirror(gpu_ctx, leaf, builder):
    """The device build (builder 1: binned-SAH topology over the Morton order, the default; builder 0: Morton radix
    tree) is a pure function of its input: the sequential host mirror gives the same nodes and records word for word."""
    hs = M.HostScene("file:coffee", 64, 36)
    gpu_ctx.set_option("leaf_size", leaf)
    gpu_ctx.set_option("builder", builder)
    try:
        gpu_ctx.load(hs)
        nodes, tris, prim = gpu_ctx.debug_read_accel()
        n64 = gpu_ctx.debug_read_nodes64()
    finally:
        gpu_ctx.set_option("builder", 1)
    hn, ht, hp, root, depth, h64 = hostsim_bvh(hs, leaf, builder, want_nodes64=True)
    info = gpu_ctx.accel_info()
    assert info.nNodes == len(hn) and info.treeDepth == depth
    assert np.array_equal(prim, hp)
    assert np.array_equal(tris[:, [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10]], ht[:, [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10]])
    assert np.array_equal(nodes[:, :29], hn[:, :29])                     # boxes, refs and child count of every Node128
    assert np.array_equal(n64, h64)                      # and of the 64-byte form the kernels fetch
    gpu_ctx.set_option("leaf_size", 4)


def test_bvh_trace_equals_oracle_closest_hit(gpu_ctx):
    hs = M.HostScene("file:coffee", 64, 36)
    gpu_ctx.load(hs)
    rng = np.random.default_rng(7)
    n = 4096
    org = rng.uniform(-1.2, 1.2, (n, 3)).astype(np.float32); org[:, 1] = rng.uniform(0.0, 0.9, n)
    d = rng.normal(size=(n, 3)).astype(np.float32); d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([org, d.astype(np.float32), np.full((n, 1), 1e-3, np.float32), np.full((n, 1), 1e27, np.float32)], axis=1)
    t, prim = gpu_ctx.debug_trace(rays)
    # every ray against the oracle's own tree (median split, built independently of the LBVH), and a sample of them
    # against the oracle's brute-force loop over all 168,193 triangles
    op, ot = oracle_scene(hs, brute_force_tris=False).closest_hits(rays)
    assert np.array_equal(prim, op)
    hit = op >= 0
    assert hit.sum() > 1000 and (~hit).sum() > 100
    assert np.array_equal(t[hit], ot[hit])
    bp, bt = oracle_scene(hs, brute_force_tris=True).closest_hits(rays[::8])
    assert np.array_equal(prim[::8], bp) and np.array_equal(t[::8][bp >= 0], bt[bp >= 0])


def test_update_video_frame_matches_oracle(gpu_ctx):
    """updateVideo (MinimalOptiX.cpp:761-778): animate, rewrite the spheres, new orbit camera, re-render."""
    import ctypes as C
    K = M._capi
    hs = M.HostScene("random_spheres", 160, 90, iarg=60)
    gpu_ctx.load(hs)
    n = hs.sizes.nSpheres
    sph = (K.SphereParams * n)()
    for i in range(n):
        sph[i] = hs.flat()["spheres"][i]
    angle = C.c_float(0.0)
    for _ in range(25):
        K.host_lib().mohost_animate_spheres(sph, n, 0.002, C.byref(angle))
    params = K.Params.from_buffer_copy(hs.params)
    K.host_lib().mohost_video_camera(angle.value, 160 / 90, C.byref(params.cam))
    gpu_ctx.update_spheres(0, sph, n)
    gpu_ctx.set_params(params)
    seeds = M.launch_seeds(2, first=100)
    gpu_ctx.accum_clear(); gpu_ctx.render(seeds)
    g = gpu_ctx.accum_read()
    d = hs.to_dict()
    d["spheres"] = np.array([[sph[i].center.x, sph[i].center.y, sph[i].center.z, sph[i].radius] for i in range(n)], np.float32)
    cam = params.cam
    d["cam"] = {k: getattr(cam, k).tolist() for k in ("origin", "horizontal", "vertical", "scrLowerLeftCorner", "u", "v")}
    d["cam"]["lensRadius"] = cam.lensRadius
    o, _ = O.Scene(d).render(seeds)
    assert rmse(g / 2, o / 2) <= RMSE_TIGHT
    assert not np.array_equal(d["spheres"], hs.to_dict()["spheres"])       # the scene really moved


def _tiny_scene(tmp_path, n_tris):
    """A file scene with n_tris triangles (n <= leaf size => the BVH root is a leaf) and one quad light."""
    d = tmp_path / "scenes" / "cornell"
    d.mkdir(parents=True)
    lines = []
    for k in range(n_tris):
        z = -0.2 * k
        lines += ["v %g -1 %g" % (-1 + 0.1 * k, z), "v %g -1 %g" % (1 + 0.1 * k, z), "v 0 1 %g" % z]
    lines += ["vn 0 0 1"]
    lines += ["f %d//1 %d//1 %d//1" % (3 * k + 1, 3 * k + 2, 3 * k + 3) for k in range(n_tris)]
    (d / "a.obj").write_text("\n".join(lines) + "\n")
    (d / "cornell.scene").write_text(
        "material M\n{\n\tcolor 0.8 0.3 0.2\n\troughness 0.4\n}\n"
        "mesh\n{\n\tfile a.obj\n\tmaterial M\n}\n"
        "light\n{\n\ttype Quad\n\tposition -1 1.5 2\n\tv1 1 1.5 2\n\tv2 -1 2.5 2.5\n\temission 5 5 5\n}\n")
    return str(tmp_path / "scenes") + "/"


@pytest.mark.parametrize("n_tris", [1, 3, 5, 9])
@pytest.mark.parametrize("variant", [0, 3, 4])
def test_tiny_meshes_root_leaf_and_shallow_trees(gpu_ctx, tmp_path, n_tris, variant):
    base = _tiny_scene(tmp_path, n_tris)
    hs = M.HostScene("file:cornell", 96, 64, base_folder=base)
    seeds = M.launch_seeds(3)
    default = gpu_ctx.get_option("kernel_variant")
    try:
        gpu_ctx.set_option("kernel_variant", variant)
        gpu_ctx.load(hs); gpu_ctx.accum_clear()
        st = gpu_ctx.render_counted(seeds)
        g = gpu_ctx.accum_read()
    finally:
        gpu_ctx.set_option("kernel_variant", default)
    o, ost = oracle_scene(hs).render(seeds)
    assert rmse(g / 3, o / 3) <= RMSE_TIGHT and st.rays == ost.rays
    assert g.max() > 0.05


def test_odd_frame_sizes_and_partitions(gpu_ctx):
    """Frames that are not multiples of the 8x8 tile, rendered whole and as 3 tile-split partitions."""
    hs = M.HostScene("file:coffee", 101, 37)
    seeds = M.launch_seeds(2)
    gpu_ctx.load(hs); gpu_ctx.accum_clear(); gpu_ctx.render(seeds)
    whole = gpu_ctx.accum_read()
    o, _ = oracle_scene(hs).render(seeds)
    assert rmse(whole / 2, o / 2) <= RMSE_TIGHT
    from minimaloptix_amd import dist as D
    parts = np.zeros_like(whole)
    try:
        for r in range(3):
            gpu_ctx.set_partition(r, 3)
            gpu_ctx.accum_clear(); gpu_ctx.render(seeds)
            a = gpu_ctx.accum_read().reshape(-1, 3)
            idx = D.tile_pixel_indices(101, 37, r, 3)
            mask = np.ones(len(a), bool); mask[idx] = False
            assert not a[mask].any()                       # a rank touches only its own tiles
            parts.reshape(-1, 3)[idx] = a[idx]
    finally:
        gpu_ctx.set_partition(0, 1)
    assert np.array_equal(parts, whole)                    # tile split is bit-identical to one GPU


@pytest.mark.parametrize("variant", [0, 3, 4])
def test_textured_scene_matches_oracle(gpu_ctx, tmp_path, variant):
    """albedo textures (rtTex2D, repeat + bilinear) on Disney and Disney-glass meshes."""
    from common import textured_scene
    hs = textured_scene(tmp_path, 128, 96)
    spp = 4
    seeds = M.launch_seeds(spp, 11)
    default = gpu_ctx.get_option("kernel_variant")
    try:
        gpu_ctx.set_option("kernel_variant", variant)
        gpu_ctx.load(hs)
        gpu_ctx.accum_clear()
        st = gpu_ctx.render_counted(seeds)
        g = gpu_ctx.accum_read()
        gpu_ctx.accum_clear()
        gpu_ctx.render(seeds)
        assert np.array_equal(gpu_ctx.accum_read(), g)
    finally:
        gpu_ctx.set_option("kernel_variant", default)
    o, ost = oracle_scene(hs).render(seeds)
    e = rmse(g / spp, o / spp)
    assert e <= RMSE_TIGHT, "paths diverged: rmse %g" % e
    assert (st.primaryRays, st.bounceRays, st.shadowRays) == (ost.primaryRays, ost.bounceRays, ost.shadowRays)
    d = hs.to_dict()
    for m in d["materials"]:
        m["albedoID"] = 0
    plain, _ = O.Scene(d).render(seeds)
    assert rmse(plain / spp, o / spp) > 1e-2          # the textures are visible in the result


def test_texture_ids_are_checked(gpu_ctx):
    import ctypes as C
    K = M._capi
    L = K.device_lib()
    L.moptix_clear_scene(gpu_ctx._h)
    m = K.Material()
    m.kind = K.MAT_DISNEY
    m.disney.albedoID = 1                                # no texture has been added yet
    assert L.moptix_add_material(gpu_ctx._h, C.byref(m), None) == K.MOPTIX_ERR_INVALID
    assert "albedoID" in gpu_ctx.last_error()
    px = np.ones((2, 2, 4), np.float32)
    tid = C.c_int32()
    assert L.moptix_add_texture(gpu_ctx._h, px.ctypes.data_as(C.POINTER(C.c_float)), 2, 2, C.byref(tid)) == K.MOPTIX_OK
    assert tid.value == 1
    assert L.moptix_add_material(gpu_ctx._h, C.byref(m), None) == K.MOPTIX_OK
    assert L.moptix_add_texture(gpu_ctx._h, None, 2, 2, None) == K.MOPTIX_ERR_INVALID
    assert L.moptix_add_texture(gpu_ctx._h, px.ctypes.data_as(C.POINTER(C.c_float)), 0, 2, None) == K.MOPTIX_ERR_INVALID
    L.moptix_clear_scene(gpu_ctx._h)


def test_full_hd_frame_properties(gpu_ctx):
    """BASELINE.json's full frame size (1920x1080) on the path bench.py times: the library's own choice of kernel (option
    kernel_variant -1: the packet kernel with the 64-byte nodes, the instantiation the benchmark runs) with 16 launches fused,
    against the oracle -- the whole frame with equal ray counts where the host has the threads for it, else a strip of 120 rows --
    and size-independent properties on the whole frame: launches accumulate linearly (seeds A then seeds B == A+B fused), an 8-way
    tile split reassembles to the 1-GPU frame bit for bit, and every ray counter is the sum of the per-partition counters."""
    import os
    W, H = 1920, 1080
    hs = M.HostScene("file:coffee", W, H)
    seeds = M.launch_seeds(16)
    assert gpu_ctx.get_option("kernel_variant") == -1 and gpu_ctx.get_option("node_format") == 0      # nothing pinned by an earlier test
    gpu_ctx.load(hs)
    gpu_ctx.accum_clear()
    st = gpu_ctx.render_counted(seeds)
    assert gpu_ctx.get_option("kernel_variant_used") == 4 and gpu_ctx.get_option("node_format_used") == 64
    gpu_ctx.accum_clear()
    gpu_ctx.render(seeds)                                      # the timed instantiation (no counters compiled in)
    whole = gpu_ctx.accum_read()
    assert gpu_ctx.get_option("kernel_variant_used") == 4 and gpu_ctx.get_option("node_format_used") == 64
    assert st.samples == W * H * 16 and st.primaryRays == st.samples
    # (1) oracle parity at the benchmark's frame size
    threads = os.cpu_count() or 1
    full = threads >= 32
    region = (0, 0, W, H) if full else (0, 480, W, 600)        # rows 480..599 run through the coffee maker and the table
    o, ost = oracle_scene(hs).render(seeds, region=region, threads=min(128, threads))
    y0, y1 = region[1], region[3]
    assert rmse(whole[y0:y1] / 16, o[y0:y1] / 16) <= 2e-6
    if full:
        assert (st.rays, st.closestHits) == (ost.rays, ost.closestHits)
    # (2) linearity over launches
    gpu_ctx.accum_clear(); gpu_ctx.render(seeds[:1]); gpu_ctx.render(seeds[1:])
    assert np.array_equal(gpu_ctx.accum_read(), whole)
    # (3) tile split x8 (the multi-GPU decomposition) == whole frame; counters add up
    from minimaloptix_amd import dist as D
    parts = np.zeros_like(whole).reshape(-1, 3)
    rays = 0
    try:
        for r in range(8):
            gpu_ctx.set_partition(r, 8)
            gpu_ctx.accum_clear()
            rays += gpu_ctx.render_counted(seeds).rays
            idx = D.tile_pixel_indices(W, H, r, 8)
            parts[idx] = gpu_ctx.accum_read().reshape(-1, 3)[idx]
    finally:
        gpu_ctx.set_partition(0, 1)
    assert np.array_equal(parts.reshape(H, W, 3), whole) and rays == st.rays


def test_work_item_order_does_not_change_the_image(gpu_ctx):
    """The hand-out order of the (pixel, sample) work items is a scheduling decision: sample-major, tile- or pixel-major
    in raster order (first launch) and with the deepest tiles / pixels first (later launches, from the recorded
    history) give the same bits, because every sample lands in its own slot of the per-sample buffer."""
    hs = M.HostScene("file:coffee", 320, 180)
    seeds = M.launch_seeds(6)
    images = []
    try:
        for tile_major, repeats in ((0, 1), (1, 3), (2, 2), (3, 3)):
            gpu_ctx.set_option("tile_major", tile_major)
            gpu_ctx.load(hs)                                  # a rebuild forgets the history
            for _ in range(repeats):
                gpu_ctx.accum_clear(); gpu_ctx.render(seeds)
                images.append(gpu_ctx.accum_read())
    finally:
        gpu_ctx.set_option("tile_major", 3)
    assert all(np.array_equal(images[0], im) for im in images[1:])
    o, _ = oracle_scene(hs).render(seeds)
    assert rmse(images[0] / 6, o / 6) <= RMSE_TIGHT


def test_randomised_option_combinations_match_variant0():
    """tools/gpu_fuzz.py: random frame sizes, sample counts, partitions and scheduler options (kernel variant, leaf
    size, work order, thresholds, workgroups per CU, multi-pass sample buffer) against the per-lane kernel."""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, CASES="40", SEED="7")
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "gpu_fuzz.py")], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "mismatches: 0 " in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]      # (tree-dependent grazing hits are counted apart: DESIGN.md section 2)


def test_random_inputs_match_the_oracle_ray_for_ray():
    """tools/gpu_oracle_fuzz.py: random scene kinds, frame sizes, sample counts, seeds, shadow rules and kernel variants through the
    C ABI against the oracle: RMSE <= 2e-6 and EQUAL counts of rays and closest hits (profiles/r04_oracle_fuzz.txt: 1,200 cases)."""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, CASES="32", SEED="9")
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "gpu_oracle_fuzz.py")], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "mismatches 0" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [0, 3, 4])
@pytest.mark.parametrize("glass_below", [True, False])
def test_shadow_rays_through_glass_nearest_any_hit_surface_decides(gpu_ctx, tmp_path, variant, glass_below):
    """Rule D5: a shadow ray is decided by its nearest any-hit surface -- a glass pane accepts it and the opaque
    pane behind never blocks.  Every kernel against the oracle, bit-level ray counts included, for both orders of the panes."""
    from common import write_glass_over_opaque_scene
    hs = M.HostScene("file:cornell", 96, 72, base_folder=write_glass_over_opaque_scene(tmp_path, glass_below))
    seeds = M.launch_seeds(6)
    default = gpu_ctx.get_option("kernel_variant")
    try:
        gpu_ctx.set_option("kernel_variant", variant)
        gpu_ctx.load(hs); gpu_ctx.accum_clear()
        st = gpu_ctx.render_counted(seeds)
        g = gpu_ctx.accum_read()
        gpu_ctx.accum_clear(); gpu_ctx.render(seeds)
        assert np.array_equal(gpu_ctx.accum_read(), g)
    finally:
        gpu_ctx.set_option("kernel_variant", default)
    o, ost = oracle_scene(hs).render(seeds)
    assert rmse(g / 6, o / 6) <= RMSE_TIGHT and st.rays == ost.rays and st.shadowRays == ost.shadowRays
    assert st.shadowRays > 0 and g.max() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [0, 3, 4])
def test_shadow_rule_0_is_survey_a2_order_independent_rule(gpu_ctx, tmp_path, variant):
    """moptix_set_option("shadow_rule", 0): the contract SURVEY A2 wrote down -- an opaque Disney surface anywhere on the segment
    blocks, every glass surface crossed multiplies -- stays available on the device (the default, 1, is the nearest-any-hit rule
    fitted to demo/coffee.png: deviation D5' in include/moptix.h).  Every kernel against the oracle's switch
    shadow_any_opaque_blocks, on the glass-over-opaque scene where the two rules give different images."""
    from common import write_glass_over_opaque_scene
    from oracle import oracle as O
    hs = M.HostScene("file:cornell", 96, 72, base_folder=write_glass_over_opaque_scene(tmp_path, True))
    seeds = M.launch_seeds(6)
    default = gpu_ctx.get_option("kernel_variant")
    imgs = {}
    try:
        gpu_ctx.set_option("kernel_variant", variant)
        for rule in (1, 0):
            gpu_ctx.set_option("shadow_rule", rule)
            assert gpu_ctx.get_option("shadow_rule") == rule
            gpu_ctx.load(hs); gpu_ctx.accum_clear()
            st = gpu_ctx.render_counted(seeds)
            imgs[rule] = (gpu_ctx.accum_read(), st)
    finally:
        gpu_ctx.set_option("shadow_rule", 1); gpu_ctx.set_option("kernel_variant", default)
    try:
        O.set_option("shadow_any_opaque_blocks", 1)
        o0, ost0 = oracle_scene(hs).render(seeds)
    finally:
        O.set_option("shadow_any_opaque_blocks", 0)
    o1, ost1 = oracle_scene(hs).render(seeds)
    g1, st1 = imgs[1]
    g0, st0 = imgs[0]
    assert rmse(g1 / 6, o1 / 6) <= RMSE_TIGHT and st1.rays == ost1.rays
    assert rmse(g0 / 6, o0 / 6) <= RMSE_TIGHT and st0.rays == ost0.rays and st0.shadowRays == ost0.shadowRays
    assert rmse(g0 / 6, g1 / 6) > 1e-3                 # the rules differ here: the opaque pane behind the glass blocks under A2


@pytest.mark.gpu
@pytest.mark.parametrize("scene,kw", [("file:coffee", {}), ("coffee_pot_standin", {}), ("dining_standin", dict(iarg=2))])
def test_node_format_changes_the_work_never_the_image(gpu_ctx, scene, kw):
    """Option node_format (variant 4): the 64-byte nodes hold every child box rounded outwards on a 256-step grid, so the
    kernel may enter more boxes than with the 128-byte nodes and must produce the same accumulator bits, the same rays and
    the same hits; the automatic choice (0) settles on one of the two, the same one every time."""
    hs = M.HostScene(scene, 160, 90, **kw)
    seeds = M.launch_seeds(16)
    res = {}
    try:
        gpu_ctx.set_option("kernel_variant", 4)
        # the packet kernel's own walk is what this test counts: the drain kernel's frontier visits a ray's boxes in whatever order its atomics
        # settle, so ITS node and triangle counts vary from run to run (its results do not: test_drain_kernel_changes_nothing)
        gpu_ctx.set_option("drain_below", 0)
        for fmt in (128, 64, 0, 0):
            gpu_ctx.set_option("node_format", fmt)
            gpu_ctx.load(hs); gpu_ctx.accum_clear()
            st = gpu_ctx.render_counted(seeds)
            assert gpu_ctx.get_option("kernel_variant_used") == 4
            used = gpu_ctx.get_option("node_format_used")
            assert used == (fmt or used) and used in (64, 128)
            res.setdefault(fmt, []).append((gpu_ctx.accum_read(), st, used))
    finally:
        gpu_ctx.set_option("node_format", 0); gpu_ctx.set_option("kernel_variant", -1); gpu_ctx.set_option("drain_below", DRAIN_DEFAULT)
    (a128, s128, _), (a64, s64, _) = res[128][0], res[64][0]
    assert np.array_equal(a128.view(np.uint32), a64.view(np.uint32))
    assert (s128.rays, s128.shadowRays, s128.closestHits) == (s64.rays, s64.shadowRays, s64.closestHits)
    assert s128.nodeFetches <= s64.nodeFetches < 1.35 * s128.nodeFetches and s128.triTests <= s64.triTests < 1.35 * s128.triTests
    (a0, s0, u0), (a1, s1, u1) = res[0]
    assert u0 == u1 and np.array_equal(a0.view(np.uint32), a128.view(np.uint32))
    assert s0.nodeFetches == (s64 if u0 == 64 else s128).nodeFetches
    o, ost = oracle_scene(hs).render(seeds[:2]) if scene == "file:coffee" else (None, None)
    if o is not None:
        gpu_ctx.set_option("kernel_variant", 4); gpu_ctx.set_option("node_format", 64)
        try:
            gpu_ctx.load(hs); gpu_ctx.accum_clear(); st = gpu_ctx.render_counted(seeds[:2])
            assert rmse(gpu_ctx.accum_read() / 2, o / 2) <= RMSE_TIGHT and st.rays == ost.rays
        finally:
            gpu_ctx.set_option("node_format", 0); gpu_ctx.set_option("kernel_variant", -1)


@pytest.mark.gpu
def test_node_format_verdicts_on_the_scenes_the_cost_model_was_fitted_to(gpu_ctx):
    """coffee (curved mesh: +2 % work under the 64-byte nodes, 3 of 7 look-ups saved) takes them.  The dining-room stand-in (walls of two
    triangles each: every ray leaving a wall starts inside the wall's quantised box, +17 % triangle tests) kept the 128-byte nodes in
    round 3 (7 % faster there), was level in round 4 (cheaper 64-byte step) and takes the 128-byte nodes again since round 5, whose
    128-byte step is fetched by the ray's signs (38.7 against 40.6 ms).  Full-size views, as profiles/r05_node_format.txt.  The
    counts, hence the verdicts, are deterministic."""
    try:
        gpu_ctx.set_option("kernel_variant", 4); gpu_ctx.set_option("node_format", 0)
        for scene, kw, want in (("file:coffee", {}, 64), ("dining_standin", dict(iarg=6), 128), ("million_standin", dict(iarg=1000000), 64)):
            hs = M.HostScene(scene, 1920, 1080, **kw)
            gpu_ctx.load(hs); gpu_ctx.accum_clear(); gpu_ctx.render(M.launch_seeds(1))
            assert gpu_ctx.get_option("node_format_used") == want, scene
    finally:
        gpu_ctx.set_option("kernel_variant", -1)


@pytest.mark.gpu
def test_a_tree_too_wide_for_the_node_grid_keeps_the_128_byte_nodes(gpu_ctx, tmp_path):
    """compress_node gives up on a node wider than 255 grid steps of 6e7 units (step/d has to stay finite for |1/d| up to 1e30):
    such a tree has no 64-byte form, the packet kernel walks the 128-byte nodes whatever node_format says, and the image is the
    per-lane kernel's."""
    from common import write_glass_over_opaque_scene
    hs = M.HostScene("file:cornell", 64, 48, base_folder=write_glass_over_opaque_scene(tmp_path, True, scale=1e10))
    seeds = M.launch_seeds(4)
    try:
        gpu_ctx.set_option("kernel_variant", 4); gpu_ctx.set_option("node_format", 64)
        gpu_ctx.load(hs); gpu_ctx.accum_clear(); gpu_ctx.render(seeds)
        assert gpu_ctx.accel_info().nNodes > 0 and gpu_ctx.get_option("node_format_used") == 128
        with pytest.raises(M.MoptixError):
            gpu_ctx.debug_read_nodes64()
        g4 = gpu_ctx.accum_read()
        gpu_ctx.set_option("kernel_variant", 0)
        gpu_ctx.accum_clear(); gpu_ctx.render(seeds)
        assert np.array_equal(g4.view(np.uint32), gpu_ctx.accum_read().view(np.uint32))
    finally:
        gpu_ctx.set_option("node_format", 0); gpu_ctx.set_option("kernel_variant", -1)


@pytest.mark.gpu
@pytest.mark.parametrize("scene,kw,size", [("file:coffee", {}, (320, 180)), ("coffee_pot_standin", {}, (200, 112)), ("dining_standin", dict(iarg=2), (200, 112)),
                                           ("million_standin", dict(iarg=3000), (200, 112))])
def test_drain_kernel_changes_nothing(gpu_ctx, scene, kw, size):
    """The launch's last paths are finished by csrc/drainkernel.hip (a wave per up to sixteen paths, all 64 lanes on one shared frontier of (node, ray)
    entries; a ray's nearest hit kept as a 64-bit (t, primitive) key under an LDS atomic minimum).  What a ray reports is defined without
    the traversal's order (rule D5), so handing paths over -- earlier or later (drain_below), whole launches of them in these small frames --
    must leave every accumulator bit, ray count and closest-hit count where the packet kernel alone (drain_below 0) puts them.  The frames are
    small on purpose: most workgroups start below the threshold and the drain kernel renders most of the image."""
    hs = M.HostScene(scene, size[0], size[1], **kw)
    seeds = M.launch_seeds(16)
    out = {}
    try:
        gpu_ctx.set_option("kernel_variant", 4)
        for db, slots in ((0, -1), (4, -1), (64, -1), (64, 64)):      # the last one: fewer slots in use than the threshold (the pool must not drain before the work items run out)
            gpu_ctx.set_option("drain_below", db); gpu_ctx.set_option("slots_in_use", slots)
            gpu_ctx.load(hs); gpu_ctx.accum_clear()
            st = gpu_ctx.render_counted(seeds)
            if gpu_ctx.get_option("kernel_variant_used") != 4:
                pytest.skip("scene outside the packet kernel's limits")
            out[(db, slots)] = (gpu_ctx.accum_read(), st)
            gpu_ctx.accum_clear(); gpu_ctx.render(seeds)                       # the uncounted instantiation
            assert np.array_equal(gpu_ctx.accum_read().view(np.uint32), out[(db, slots)][0].view(np.uint32))
    finally:
        gpu_ctx.set_option("drain_below", DRAIN_DEFAULT); gpu_ctx.set_option("kernel_variant", -1); gpu_ctx.set_option("slots_in_use", -1)
    a0, s0 = out[(0, -1)]
    for db in ((4, -1), (64, -1), (64, 64)):
        a, st = out[db]
        assert np.array_equal(a.view(np.uint32), a0.view(np.uint32)), "drain_below / slots_in_use %s changed the image" % (db,)
        assert (st.rays, st.shadowRays, st.closestHits, st.samples) == (s0.rays, s0.shadowRays, s0.closestHits, s0.samples)


@pytest.mark.gpu
@pytest.mark.parametrize("leaf,builder", [(1, 1), (4, 1), (8, 1), (4, 0)])
def test_every_child_box_contains_its_triangles(gpu_ctx, leaf, builder):
    """the fuzzers excuse a difference between two trees as a tree-dependent grazing hit when the simplest kernel reproduces it on
    the candidate's tree -- which a builder bug (a box that does not enclose its triangles) would pass as well.  So the trees themselves are
    checked: every child box, in the 128-byte form and in the decoded 64-byte form the kernels fetch, contains all triangles below it."""
    for scene, kw in (("million_standin", dict(iarg=3000)), ("file:coffee", {})):
        hs = M.HostScene(scene, 64, 36, **kw)
        gpu_ctx.set_option("leaf_size", leaf); gpu_ctx.set_option("builder", builder)
        try:
            gpu_ctx.load(hs)
            nodes, tris, _prim = gpu_ctx.debug_read_accel()
            n64 = gpu_ctx.debug_read_nodes64()
            root = 0 if len(nodes) else -1
        finally:
            gpu_ctx.set_option("builder", 1); gpu_ctx.set_option("leaf_size", 4)
        assert len(nodes) > 0
        assert tree_containment_errors(nodes, tris, root, n64) == 0, (scene, leaf, builder)


@pytest.mark.gpu
def test_the_known_grazing_hit_is_tree_dependent_and_nothing_else(gpu_ctx):
    """the one accepted GPU-against-oracle difference, replayed (tools/gpu_oracle_fuzz.py seed 58 case 62: the 3,000-face glass
    knot, 200x112, 2 spp).  The reference's float triangle test (Geometry.cu:121-160 = pt_geom.h tri_test) accepts a grazing hit on a needle
    triangle at a point outside that triangle's own box; whether a traversal ever tests the triangle depends on the boxes around it (rule D5's
    one exception, include/moptix.h).  The three legs of the proof, asserted:
      (1) the CPU build of the kernel's own code on the device's tree gives the GPU's counts and image: the GPU executes the specified algorithm;
      (2) on ANOTHER tree of the same triangles (the 64-byte nodes, whose boxes are supersets) the GPU gives exactly the oracle's;
      (3) the oracle's brute-force mode agrees with the oracle's tree: the oracle's answer is the order-free one;
    and the damage is bounded: one pixel-sample, RMSE <= 1e-3 (north_star's bar), every other pixel to RMSE_TIGHT."""
    hs = M.HostScene("million_standin", 200, 112, iarg=3000)
    seeds = M.launch_seeds(2, 67078)
    o, ost = oracle_scene(hs).render(seeds)
    ob, obst = oracle_scene(hs, brute_force_tris=True).render(seeds)
    assert obst.closestHits == ost.closestHits and obst.rays == ost.rays and rmse(o / 2, ob / 2) <= RMSE_TIGHT            # leg 3
    out = {}
    try:
        for fmt in (128, 64):
            gpu_ctx.set_option("kernel_variant", 4); gpu_ctx.set_option("node_format", fmt)
            gpu_ctx.load(hs); gpu_ctx.accum_clear()
            st = gpu_ctx.render_counted(seeds)
            out[fmt] = (gpu_ctx.accum_read(), st)
        nodes, tris, _prim = gpu_ctx.debug_read_accel()
        assert tree_containment_errors(nodes, tris, 0, gpu_ctx.debug_read_nodes64()) == 0                                 # the tree itself is valid
    finally:
        gpu_ctx.set_option("node_format", 0); gpu_ctx.set_option("kernel_variant", -1)
    g128, s128 = out[128]; g64, s64 = out[64]
    assert s64.closestHits == ost.closestHits and s64.rays == ost.rays and rmse(g64 / 2, o / 2) <= RMSE_TIGHT              # leg 2
    h128, hc = hostsim_render(hs, seeds, node_format=128)
    assert hc["closestHits"] == s128.closestHits and rmse(h128 / 2, g128 / 2) <= RMSE_TIGHT                                # leg 1
    # the damage: one closest hit more, one pixel, inside north_star's bound
    assert s128.closestHits == ost.closestHits + 1
    d = np.abs(g128.astype(np.float64) - o.astype(np.float64)).max(axis=-1)
    assert int((d > 1e-5).sum()) == 1 and rmse(g128 / 2, o / 2) <= 1e-3
    keep = d <= 1e-5
    assert rmse((g128 / 2)[keep], (o / 2)[keep]) <= RMSE_TIGHT


def test_bench_dump_outputs_is_the_frame_the_library_renders(gpu_ctx, tmp_path):
    """`bench.py --dump-outputs DIR`, plain and with --full (whose side legs render into the same buffer after the timed frames): DIR/accum.npy is
    the last timed frame, bit for bit the accumulation buffer the library gives for the same scene and seeds."""
    import json
    import os
    import subprocess
    import sys
    from common import REPO
    W, H, spp = 160, 90, 4
    got = {}
    for name, extra in (("plain", []), ("full", ["--full", "--no-cpu-baseline"])):
        d = tmp_path / name
        p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--width", str(W),
                            "--height", str(H), "--spp", str(spp), "--dump-outputs", str(d)] + extra, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-2000:])
        line = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
        assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["outputs"]["arrays"] == {"accum": [H, W, 3]}
        assert ("fast_shading_mode" in line) == (name == "full")
        got[name] = np.load(d / "accum.npy")
    gpu_ctx.load(M.HostScene("file:coffee", W, H))
    gpu_ctx.accum_clear()
    gpu_ctx.render(M.launch_seeds(spp))
    ref = gpu_ctx.accum_read()
    assert ref.any() and np.array_equal(got["plain"], ref) and np.array_equal(got["full"], ref)

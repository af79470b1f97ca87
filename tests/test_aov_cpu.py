"""First-hit AOVs (include/moptix.h "first-hit AOVs") without a GPU: the CPU mirror of the AOV kernel (tests/hostsim/aovsim.cpp, the kernel's own
per-pixel code from pt_aov.h) against the oracle and against the semantics table, and the C ABI's boundary errors."""
import ctypes as C
import os

import numpy as np
import pytest

from common import M, K, O, have_gpu, oracle_scene, textured_scene, write_png
from aov_helpers import aovsim_render, camera_rays, empty_aovs

W, H = 64, 36


def _scene(kind, tmp_path, w=W, h=H):
    if kind == "textured":
        return textured_scene(tmp_path, w, h)
    return M.HostScene(kind, w, h)


@pytest.mark.parametrize("kind", ["spheres", "cornell_quads", "file:coffee", "textured"])
def test_camera_rays_through_the_oracle_give_the_aov_ids_and_depth(kind, tmp_path):
    """aovsim's camera rays (begin_sample's) through the oracle's closest-hit query: the same primitive and, one seed, the same depth bits."""
    hs = _scene(kind, tmp_path)
    seed = int(M.launch_seeds(1)[0])
    a = aovsim_render(hs, [seed])
    prim, t = oracle_scene(hs).closest_hits(camera_rays(hs, seed))
    assert np.array_equal(a["primId"].reshape(-1), prim)
    hit = prim >= 0
    assert hit.any()
    assert np.array_equal(a["hits"].reshape(-1), hit.astype(np.float32))
    assert np.array_equal(a["depth"].reshape(-1)[hit].view(np.uint32), t[hit].view(np.uint32))
    assert not a["depth"].reshape(-1)[~hit].any()
    mats = np.asarray(oracle_material_ids(hs))
    assert np.array_equal(a["matId"].reshape(-1)[hit], mats[prim[hit]]) and (a["matId"].reshape(-1)[~hit] == -1).all()


def oracle_material_ids(hs):
    """material of every primitive id (spheres, quads, triangles in upload order)"""
    f = hs.flat()
    return list(f["sphereMat"]) + list(f["quadMat"]) + list(f["faceMat"])


def _material(hs, i):
    return hs.flat()["materials"][i]


def test_albedo_of_lambertian_metal_glass_is_the_material_albedo():
    hs = M.HostScene("spheres", W, H)
    a = aovsim_render(hs, M.launch_seeds(1))
    mat = a["matId"][..., 0]
    miss = a["primId"][..., 0] < 0
    kinds = set()
    for m in np.unique(mat[~miss]):
        mm = _material(hs, int(m))
        if mm.kind in (K.MAT_LAMBERTIAN, K.MAT_METAL, K.MAT_GLASS):
            kinds.add(int(mm.kind))
            assert (a["albedo"][mat == m] == np.float32([mm.albedo.x, mm.albedo.y, mm.albedo.z])).all(), int(m)
    assert kinds == {K.MAT_LAMBERTIAN, K.MAT_METAL, K.MAT_GLASS}


def _single_colour_scene(root, rgb):
    d = os.path.join(str(root), "cornell")
    os.makedirs(d, exist_ok=True)
    write_png(os.path.join(d, "flat.png"), np.tile(np.uint8(rgb), (2, 2, 1)))
    with open(os.path.join(d, "back.obj"), "w") as f:
        f.write("v -1 -1 1\nv -1 1 1\nv 1 1 1\nv 1 -1 1\nvt 0.1 0.2\nvt 0.3 2.7\nvt -1.6 0.9\nvt 0.5 0.5\nf 1/1 2/2 3/3 4/4\n")
    with open(os.path.join(d, "floor.obj"), "w") as f:          # gives the scene its extent (the camera is placed from it)
        f.write("v -1 -1 -1\nv -1 -1 1\nv 1 -1 1\nv 1 -1 -1\nf 1 2 3 4\n")
    with open(os.path.join(d, "cornell.scene"), "w") as f:
        f.write("material Back\n{\n    color 0.2 0.9 0.4\n    albedoTex flat.png\n    roughness 0.5\n}\n"
                "material Floor\n{\n    color 0.5 0.5 0.5\n}\n"
                "mesh\n{\n    file back.obj\n    material Back\n}\n"
                "mesh\n{\n    file floor.obj\n    material Floor\n}\n"
                "light\n{\n    type Quad\n    position -0.4 0.98 -0.4\n    v1 0.4 0.98 -0.4\n    v2 -0.4 0.98 0.4\n    emission 12 12 12\n}\n")
    return M.HostScene("file:cornell", W, H, base_folder=str(root) + "/")


def test_albedo_of_a_textured_disney_hit_is_the_linearised_texel_and_a_miss_the_background(tmp_path):
    hs = _single_colour_scene(tmp_path, [200, 90, 30])
    texel = hs.flat()["textures"][0][0, 0, :3].astype(np.float32)
    want = np.array([np.float32(np.power(np.float64(c), np.float64(np.float32(2.2)))) for c in texel], np.float32)
    a = aovsim_render(hs, M.launch_seeds(3))
    back = a["matId"][..., 0] == 0                     # the first sample hit the textured wall ...
    hit = back & (a["hits"][..., 0] == 3) & (a["albedo"][..., 0] == (want[0] + want[0]) + want[0])
    assert back.sum() > 100 and hit.sum() >= 0.9 * back.sum()      # ... and (nearly everywhere) so did the other two
    assert (a["albedo"][hit] == (want + want) + want).all()          # three samples summed in seed order
    one = aovsim_render(hs, M.launch_seeds(1))
    b1 = one["matId"][..., 0] == 0
    assert b1.sum() > 100 and (one["albedo"][b1] == want).all()
    # and a miss is the background colour
    bg = np.float32([hs.params.bgColor.x, hs.params.bgColor.y, hs.params.bgColor.z])
    miss = one["primId"][..., 0] < 0
    assert miss.any() and (one["albedo"][miss] == bg).all()


@pytest.mark.parametrize("kind", ["spheres", "cornell_quads", "file:coffee", "textured"])
def test_normals_are_unit_and_face_the_camera_on_analytic_scenes(kind, tmp_path):
    hs = _scene(kind, tmp_path)
    seed = int(M.launch_seeds(1)[0])
    a = aovsim_render(hs, [seed])
    hit = a["primId"].reshape(-1) >= 0
    n = a["normal"].reshape(-1, 3)[hit].astype(np.float64)
    assert np.abs(np.linalg.norm(n, axis=1) - 1.0).max() <= 1e-6
    assert not a["normal"].reshape(-1, 3)[~hit].any()
    if kind in ("spheres", "cornell_quads"):        # shading normal = geometric normal there; mesh normals may lean past the silhouette
        d = camera_rays(hs, seed)[hit, 3:6].astype(np.float64)
        assert ((n * d).sum(axis=1) <= 0).all()


@pytest.mark.parametrize("kind,node_format", [("file:coffee", 64), ("file:coffee", 128), ("spheres", 64)])
def test_two_calls_give_the_bits_of_one(kind, node_format):
    hs = M.HostScene(kind, W, H)
    seeds = M.launch_seeds(5, 11)
    whole = aovsim_render(hs, seeds, node_format=node_format)
    parts = aovsim_render(hs, seeds[:2], node_format=node_format)
    parts = aovsim_render(hs, seeds[2:], node_format=node_format, aovs=parts)
    assert whole["samples"] == parts["samples"] == 5
    for n in ("albedo", "normal", "depth", "hits", "primId", "matId"):
        assert np.array_equal(whole[n].view(np.uint32), parts[n].view(np.uint32)), n
    first = aovsim_render(hs, seeds[:1], node_format=node_format)
    assert np.array_equal(whole["primId"], first["primId"]) and np.array_equal(whole["matId"], first["matId"])   # ids: first sample only


def test_aov_entries_reject_a_null_context():
    lib = K.device_lib()
    seeds = (C.c_int32 * 1)(0)
    n = C.c_uint64()
    b = K.AovBuffers()
    assert lib.moptix_render_aovs(None, seeds, 1) == K.ERR_INVALID
    assert lib.moptix_aov_clear(None) == K.ERR_INVALID
    assert lib.moptix_aov_samples(None, C.byref(n)) == K.ERR_INVALID
    assert lib.moptix_aov_read(None, C.byref(b)) == K.ERR_INVALID
    assert lib.moptix_aov_bind(None, C.byref(b)) == K.ERR_INVALID


@pytest.mark.skipif(have_gpu(), reason="checks the no-device error path")
def test_no_aovs_without_a_device(tmp_path):
    """No CPU path for the AOVs either: without a device there is no context to render them with, and the CLI's --aov fails loudly."""
    import subprocess
    from common import REPO
    with pytest.raises(M.MoptixError) as e:
        M.Context(0).render_aovs([0])
    assert e.value.code == K.ERR_NO_DEVICE
    p = subprocess.run([os.path.join(REPO, "minimaloptix_amd", "lib", "moptix_render"), "--scene", "spheres", "--width", "32", "--height", "16",
                        "--spp", "1", "--aov", "--scenes", os.path.join(REPO, "scenes") + "/", "--outdir", str(tmp_path)],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and not list(tmp_path.glob("*.pfm"))

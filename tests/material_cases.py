"""Material cases for the Disney code (csrc/pt_disney.h, its callers in pt_path.h and pt_packet.h, the records of pt_upload.h): the
floor / back-wall / block scene of packet_helpers.write_floor_block_scene with its two material blocks written from dicts, so that every
one of the ten Disney parameters is away from its default somewhere and at 0 and at 1 somewhere, and three further scenes: twelve
materials on small faces, a Disney GLASS pane, a plain Lambertian panel.  Every parameter stays inside [0, 1].

A material is a dict of the keys of PARAMS plus "color" and "brdf"; what it leaves out keeps the scene file's default (DEFAULTS).  The
Block keeps the colour (0.8, 0.3, 0.2) and the Floor (which the back wall shares) (0.7, 0.7, 0.7) unless a case says otherwise."""
import tempfile
from pathlib import Path

import numpy as np

from common import K, M, MovedScene
from packet_helpers import write_floor_block_scene

PARAMS = ("metallic", "subsurface", "specular", "roughness", "specularTint", "anisotropic", "sheen", "sheenTint", "clearcoat", "clearcoatGloss")
DEFAULTS = dict(metallic=0.0, subsurface=0.0, specular=0.5, roughness=0.5, specularTint=0.0, anisotropic=0.0, sheen=0.0, sheenTint=0.5,
                clearcoat=0.0, clearcoatGloss=1.0)      # host/scene_file.cpp initDisneyParams
BLOCK_COLOR, FLOOR_COLOR = (0.8, 0.3, 0.2), (0.7, 0.7, 0.7)

ALL_BLOCK = dict(metallic=0.3, subsurface=0.4, specular=0.8, roughness=0.25, specularTint=0.6, anisotropic=0.7, sheen=0.5, sheenTint=0.2,
                 clearcoat=0.6, clearcoatGloss=0.3)
ALL_FLOOR = dict(color=(0.6, 0.7, 0.5), metallic=0.15, subsurface=0.65, specular=0.2, roughness=0.45, specularTint=0.35, anisotropic=0.4,
                 sheen=0.8, sheenTint=0.75, clearcoat=0.3, clearcoatGloss=0.6)

# name -> (Block, Floor)
PAIRS = {
    "aniso": (dict(roughness=0.3, anisotropic=0.8), dict(roughness=0.4, anisotropic=1.0)),
    "subsurf": (dict(roughness=0.5, subsurface=0.7), dict(roughness=0.6, subsurface=1.0)),
    "sheen": (dict(sheen=1.0, sheenTint=0.9), dict(color=(0.2, 0.7, 0.7), sheen=0.5, sheenTint=0.0)),
    "ccgloss": (dict(roughness=0.3, clearcoat=1.0, clearcoatGloss=0.2), dict(clearcoat=0.7, clearcoatGloss=0.0)),
    "metal1": (dict(roughness=0.2, metallic=1.0), dict(roughness=0.0, metallic=0.9)),
    "rough0": (dict(roughness=0.0), dict(roughness=1.0)),
    "spec": (dict(specular=1.0, specularTint=1.0), dict(color=(0.0, 0.0, 0.0), specular=0.0)),
    "black": (dict(color=(0.0, 0.0, 0.0), specularTint=1.0, sheen=1.0, sheenTint=1.0), dict(color=(1.0, 1.0, 1.0))),
    "all": (ALL_BLOCK, ALL_FLOOR),
}
PAIR_NAMES = tuple(PAIRS)
TWELVE, GLASS, LAMBERTIAN = "twelve", "glass", "lambertian"
CASE_NAMES = PAIR_NAMES + (TWELVE, GLASS, LAMBERTIAN)
GRAZING_CASES = ("all", "rough0", "aniso", "metal1", "ccgloss")
GRAZING_ELEVATIONS = (1e-1, 1e-2, 1e-3, 1e-4, 1e-5)
GRAZING_N = 512

GLASS_PANE = dict(color=(0.9, 0.8, 0.7), brdf=1, metallic=0.2, subsurface=0.3, specular=0.9, roughness=0.35, specularTint=0.4, anisotropic=0.5,
                  sheen=0.6, sheenTint=0.1, clearcoat=0.8, clearcoatGloss=0.4)
LAMBERTIAN_ALBEDO = (0.2, 0.6, 0.8)
# the block's five faces as block.obj winds them (corner, corner + du, ., corner + dv)
_BLOCK_V = np.array([[-0.5, 0, -0.5], [0.5, 0, -0.5], [0.5, 0, 0.5], [-0.5, 0, 0.5], [-0.5, 0.8, -0.5], [0.5, 0.8, -0.5], [0.5, 0.8, 0.5], [-0.5, 0.8, 0.5]])
_BLOCK_F = ((5, 8, 7, 6), (1, 2, 6, 5), (2, 3, 7, 6), (3, 4, 8, 7), (4, 1, 5, 8))
_BLOCK_CELLS, _FLOOR_CELLS = 5, (12, 8)


def block_material(m):
    return dict(dict(color=BLOCK_COLOR), **m)


def floor_material(m):
    return dict(dict(color=FLOOR_COLOR), **m)


def twelve_materials():
    """Twelve parameter vectors from a fixed seed, uniform in [0, 1]^10 with colours in [0.1, 0.9]^3; the first five are pushed to an end
    point each, so that lanes side by side differ in diffuseRatio, ccRatio, ccAlpha, the ax / ay floors and the subsurface lerp."""
    rng = np.random.default_rng(1201)
    out = []
    for k in range(12):
        m = dict(zip(PARAMS, np.round(rng.uniform(0.0, 1.0, len(PARAMS)), 3).tolist()))
        m["color"] = tuple(np.round(rng.uniform(0.1, 0.9, 3), 3).tolist())
        out.append(m)
    out[0]["roughness"] = 0.0
    out[1]["metallic"] = 1.0
    out[2]["anisotropic"] = 1.0; out[2]["roughness"] = 0.3
    out[3]["subsurface"] = 1.0
    out[4]["clearcoat"] = 1.0; out[4]["clearcoatGloss"] = 0.0
    return out


def case_materials(name):
    """The Disney materials of a case as full dicts (every key of PARAMS, "color", "brdf"), in the scene's material order."""
    if name in PAIRS:
        mats = [floor_material(PAIRS[name][1]), block_material(PAIRS[name][0])]
    elif name == TWELVE:
        mats = [floor_material(ALL_FLOOR)] + twelve_materials()
    elif name == GLASS:
        mats = [floor_material(ALL_FLOOR), block_material(ALL_BLOCK), dict(GLASS_PANE)]
    else:
        mats = [floor_material(ALL_FLOOR), block_material(ALL_BLOCK)]      # the Lambertian panel is no Disney material
    return [dict(dict(DEFAULTS, brdf=0), **m) for m in mats]


def material_text(name, m):
    """A material block of a .scene file.  One key per line: a line gives a value to every key whose format it matches, and
    "specular" / "sheen" / "clearcoat" match the start of their longer neighbours' lines without taking a number from them."""
    lines = ["\tcolor %.9g %.9g %.9g" % tuple(m.get("color", (1.0, 1.0, 1.0)))]
    lines += ["\t%s %.9g" % (k, m[k]) for k in PARAMS if k in m]
    if m.get("brdf", 0):
        lines.append("\tbrdf %d" % m["brdf"])
    return "material %s\n{\n%s\n}\n" % (name, "\n".join(lines))


def _cells(corner, du, dv, nu, nv):
    """The nu x nv cells of the parallelogram corner, corner + du, corner + du + dv, corner + dv, each wound as the whole is."""
    for i in range(nu):
        for j in range(nv):
            p = corner + du * (i / nu) + dv * (j / nv)
            yield i, j, (p, p + du / nu, p + du / nu + dv / nv, p + dv / nv)


def _write_twelve_objs(d):
    """mat00.obj .. mat11.obj: the block's five faces cut into 5 x 5 cells (no normals) and the floor into 12 x 8 (normal +y), dealt out
    so that neighbouring cells never share a material; wall.obj: the back wall."""
    files = [[] for _ in range(12)]
    for f, (a, b, _c, e) in enumerate(_BLOCK_F):
        corner = _BLOCK_V[a - 1]
        for i, j, quad in _cells(corner, _BLOCK_V[b - 1] - corner, _BLOCK_V[e - 1] - corner, _BLOCK_CELLS, _BLOCK_CELLS):
            files[(i + 5 * j + 3 * f) % 12].append((quad, False))
    corner = np.array([-3.0, 0.0, -2.0])
    for i, j, quad in _cells(corner, np.array([0.0, 0.0, 4.0]), np.array([6.0, 0.0, 0.0]), _FLOOR_CELLS[1], _FLOOR_CELLS[0]):
        files[(i + 5 * j) % 12].append((quad, True))
    for k, quads in enumerate(files):
        lines = ["vn 0 1 0"]
        for q, (quad, with_normal) in enumerate(quads):
            lines += ["v %.9g %.9g %.9g" % tuple(p) for p in quad]
            lines.append("f " + " ".join(("%d//1" if with_normal else "%d") % (4 * q + c + 1) for c in range(4)))
        (d / ("mat%02d.obj" % k)).write_text("\n".join(lines) + "\n")
    (d / "wall.obj").write_text("v -3 0 2\nv -3 3.4 2\nv 3 3.4 2\nv 3 0 2\nvn 0 0 -1\nf 1//1 2//1 3//1 4//1\n")


LIGHT_TEXT = "light\n{\n\ttype Quad\n\tposition -1 2.5 -1\n\tv1 0 2.5 -1\n\tv2 -1 2.5 0\n\temission 12 12 12\n}\n"


def write_case_scene(root, name, tilted_normals=False):
    """The case's files under root/scenes/cornell; returns the base folder for M.HostScene("file:cornell", ...)."""
    root = Path(root)
    base = write_floor_block_scene(root, tilted_normals=tilted_normals)      # floor.obj (floor and back wall), block.obj; its .scene is replaced
    d = root / "scenes" / "cornell"
    if name in PAIRS:
        mats = [("Floor", floor_material(PAIRS[name][1])), ("Block", block_material(PAIRS[name][0]))]
        meshes = [("floor.obj", "Floor"), ("block.obj", "Block")]
    elif name == TWELVE:
        _write_twelve_objs(d)
        mats = [("Floor", floor_material(ALL_FLOOR))] + [("M%02d" % k, m) for k, m in enumerate(twelve_materials())]
        meshes = [("wall.obj", "Floor")] + [("mat%02d.obj" % k, "M%02d" % k) for k in range(12)]
    else:
        mats = [("Floor", floor_material(ALL_FLOOR)), ("Block", block_material(ALL_BLOCK))]
        meshes = [("floor.obj", "Floor"), ("block.obj", "Block")]
        if name == GLASS:
            # a tilted pane between the light and the floor, left of the block: seen by the camera, met by shadow rays and by bounces
            (d / "pane.obj").write_text("v -2.2 0.9 -1.6\nv 0.2 0.9 -1.6\nv 0.2 2 0.2\nv -2.2 2 0.2\nf 1 3 2\nf 1 4 3\n")
            mats.append(("Pane", GLASS_PANE)); meshes.append(("pane.obj", "Pane"))
        elif name == LAMBERTIAN:
            # a tilted panel in front of the back wall, left of the block; case_scene makes its material a Lambertian one
            (d / "panel.obj").write_text("v -2.2 0.2 1.2\nv -2.2 1.6 1.5\nv -1 1.6 1.5\nv -1 0.2 1.2\nf 1 2 3\nf 1 3 4\n")
            mats.append(("Panel", dict(color=LAMBERTIAN_ALBEDO))); meshes.append(("panel.obj", "Panel"))
        else:
            raise KeyError(name)
    (d / "cornell.scene").write_text("".join(material_text(n, m) for n, m in mats) +
                                     "".join("mesh\n{\n\tfile %s\n\tmaterial %s\n}\n" % fm for fm in meshes) + LIGHT_TEXT)
    return base


_scenes = {}


def case_scene(name, width=96, height=54, tilted_normals=False):
    """The case as a scene (made once per size: the tests only read it).  The Lambertian case is the file's scene over a copy of its
    flat arrays, with the panel's material record replaced: a .scene file has Disney materials only."""
    key = (name, width, height, tilted_normals)
    if key not in _scenes:
        with tempfile.TemporaryDirectory() as tmp:
            hs = M.HostScene("file:cornell", width, height, base_folder=write_case_scene(tmp, name, tilted_normals))
        assert not hs.warnings, hs.warnings
        if name == LAMBERTIAN:
            hs = MovedScene(hs)
            mats = (K.Material * hs.sizes.nMaterials).from_buffer_copy(hs.flat()["materials"])
            panel = K.Material()
            panel.kind = K.MAT_LAMBERTIAN
            panel.albedo = K.Float3(*LAMBERTIAN_ALBEDO); panel.refIdx = 1.0
            mats[int(hs.flat()["faceMat"][-1])] = panel      # the panel is the last mesh; the light's material follows the meshes'
            hs.flat()["materials"] = mats
        _scenes[key] = hs
    return _scenes[key]


def scene_material(hs, i):
    """Material record i of a scene, as moptix_add_material takes it."""
    return K.Material.from_buffer_copy(hs.flat()["materials"][i])


def grazing_rays(hs, elevation, n, rng):
    """n rays (o, d, tmin, tmax) towards uniformly drawn points of the floor (y = 0, x in -3 .. 3, z in -2 .. 2), `elevation` radians
    above its plane from a uniformly drawn side, starting 0.2 .. 1 away from the point.  The directions are renormalised in binary32;
    tmin is the scene's rayEpsilonT, tmax 1e27."""
    p = np.stack([rng.uniform(-3.0, 3.0, n), np.zeros(n), rng.uniform(-2.0, 2.0, n)], axis=1)
    phi = rng.uniform(0.0, 2.0 * np.pi, n)
    d = np.stack([np.cos(elevation) * np.cos(phi), np.full(n, -np.sin(elevation)), np.cos(elevation) * np.sin(phi)], axis=1)
    o = (p - rng.uniform(0.2, 1.0, n)[:, None] * d).astype(np.float32)
    d = d.astype(np.float32)
    d = (d / np.sqrt((d * d).sum(axis=1, dtype=np.float32), dtype=np.float32)[:, None]).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([o, d, np.full((n, 1), hs.params.rayEpsilonT, np.float32), np.full((n, 1), 1e27, np.float32)],
                                               axis=1))


def grazing_sets(hs, seed=31):
    """The grazing rays of a scene, elevation -> (GRAZING_N, 8): one generator, the elevations in GRAZING_ELEVATIONS' order."""
    rng = np.random.default_rng(seed)
    return {e: grazing_rays(hs, e, GRAZING_N, rng) for e in GRAZING_ELEVATIONS}

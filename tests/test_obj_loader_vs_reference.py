"""The repo's own .obj loader against the reference's vendored tiny_obj_loader.h v1.4.0 (MinimalOptiX/tiny_obj_loader.h).
Same dump program around both (oracle/obj_dump.cpp): the attribute arrays and every (vertex, normal, texcoord) index must
agree byte for byte -- this is MinimalOptiX.cpp:385's LoadObj call, the one piece of the reference on this path that CAN be run.

What tinyobj dumps for each input is recorded in tests/golden/tinyobj_dumps.json (size + SHA-256 of the dump), so the comparison
runs wherever the repository does.  Where oracle/Makefile could also build the reference's loader (oracle/_ref/tinyobj_dump, made
only where the reference's header is present, never committed), each dump is in addition compared with that binary's live output
and with the record.  `python tests/test_obj_loader_vs_reference.py` rewrites the record from that binary."""
import glob
import hashlib
import json
import os
import subprocess
import sys

import pytest

from common import M, REPO

REF = os.path.join(REPO, "oracle", "_ref", "tinyobj_dump")
OURS = os.path.join(REPO, "oracle", "mobj_dump")
RECORD = os.path.join(REPO, "tests", "golden", "tinyobj_dumps.json")


def _dump(exe, obj, out):
    r = subprocess.run([exe, obj, out], capture_output=True, text=True)
    return r.returncode, (open(out, "rb").read() if r.returncode == 0 else r.stderr)


def _digest(b):
    return {"bytes": len(b), "sha256": hashlib.sha256(b).hexdigest()}


def _ours():
    if not os.path.exists(OURS):
        subprocess.check_call(["make", "-C", os.path.join(REPO, "oracle"), "-s", "mobj_dump"])
    return OURS


def _check_like_tinyobj(key, path, tmp_path):
    """Our dump of `path` against tinyobj's: the recorded digest always, the live reference build where it exists."""
    rc2, b = _dump(_ours(), path, str(tmp_path / "b.bin"))
    assert rc2 == 0, (key, b)
    want = json.load(open(RECORD))[key]
    assert _digest(b) == want, key
    if os.path.exists(REF):
        rc1, a = _dump(REF, path, str(tmp_path / "a.bin"))
        assert rc1 == 0, (key, a)
        assert a == b and _digest(a) == want, key


def _coffee_meshes():
    return sorted(glob.glob(os.path.join(M.scenes_dir(), "coffee", "Mesh*.obj")))


def test_every_coffee_mesh_loads_like_tinyobj(tmp_path):
    meshes = _coffee_meshes()
    assert len(meshes) == 19
    for m in meshes:
        _check_like_tinyobj("coffee/" + os.path.basename(m), m, tmp_path)


CASES = {
    "quad_fan": "v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvn 0 0 1\nvt 0.5 0.25\nf 1/1/1 2/1/1 3/1/1 4/1/1\n",
    "pentagon": "v 0 0 0\nv 1 0 0\nv 1.5 1 0\nv 0.5 2 0\nv -0.5 1 0\nf 1 2 3 4 5\n",
    "negative_indices": "v 0 0 0\nv 1 0 0\nv 0 1 0\nvn 0 0 1\nf -3//-1 -2//-1 -1//-1\nv 2 0 0\nf -1 -3 -2\n",
    "mixed_forms": "v 0 0 0\nv 1 0 0\nv 0 1 0\nv 1 1 0\nvt 0 0\nvt 1 0\nvt 0 1\nvn 0 0 1\nf 1/1 2/2 3/3\nf 2//1 4//1 3//1\nf 1 2 4\n",
    "groups_and_objects": "o a\nv 0 0 0\nv 1 0 0\nv 0 1 0\ng g1\nf 1 2 3\ng g2\nv 0 0 1\nf 1 2 4\no b\nf 2 3 4\n",
    "comments_blank_crlf": "# c\r\n\r\nv 0 0 0\r\nv 1 0 0\r\nv 0 1 0\r\nmtllib x.mtl\r\nusemtl m\r\ns off\r\nf 1 2 3\r\n",
    "whitespace": "v   0.5\t-1e-3   2.5E+1\nv 1 0 0\nv 0 1 0\nf   1   2   3  \n",
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_obj_syntax_cases_load_like_tinyobj(tmp_path, name):
    p = tmp_path / (name + ".obj")
    p.write_bytes(CASES[name].encode())
    _check_like_tinyobj("case/" + name, str(p), tmp_path)


def _record():
    """Rewrites RECORD from the reference's loader (oracle/_ref/tinyobj_dump)."""
    import tempfile
    d = tempfile.mkdtemp()
    out = {}
    inputs = [("coffee/" + os.path.basename(m), m) for m in _coffee_meshes()]
    for name in sorted(CASES):
        p = os.path.join(d, name + ".obj")
        with open(p, "wb") as f:
            f.write(CASES[name].encode())
        inputs.append(("case/" + name, p))
    for key, path in inputs:
        rc, a = _dump(REF, path, os.path.join(d, "a.bin"))
        assert rc == 0, (key, a)
        out[key] = _digest(a)
    with open(RECORD, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    sys.exit(_record())

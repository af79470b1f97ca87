"""Scene helpers for the face-motion tests (the mirror is temporal_helpers.TemporalSim with its option on)."""
import numpy as np

from common import M, MovedScene


def first_face(hs):
    """primId of face 0: ids are spheres, quads, triangles in upload order."""
    return int(hs.sizes.nSpheres) + int(hs.sizes.nQuads)


def translated(face_pos, offset):
    """(nFaces, 9) float32: every vertex moved by `offset`, one binary32 addition per component."""
    fp = np.asarray(face_pos, np.float32).reshape(-1, 3, 3)
    return (fp + np.asarray(offset, np.float32)[None, None, :]).astype(np.float32).reshape(-1, 9)


def grid_mesh_scene(nx, ny, x0, x1, y0, y1, z, width=64, height=36):
    """A flat nx x ny grid of quads, two triangles each, in the plane at depth `z` of coffee's frame (its camera, materials and lights;
    none of its own faces): triangles a few pixels wide when nx, ny are large.  Returns the MovedScene."""
    xs = np.linspace(x0, x1, nx + 1, dtype=np.float32); ys = np.linspace(y0, y1, ny + 1, dtype=np.float32)
    faces = []
    for j in range(ny):
        for i in range(nx):
            a, b, c, d = (xs[i], ys[j], z), (xs[i + 1], ys[j], z), (xs[i + 1], ys[j + 1], z), (xs[i], ys[j + 1], z)
            faces.append(a + b + c); faces.append(a + c + d)
    return MovedScene(M.HostScene("file:coffee", width, height), np.asarray(faces, np.float32), new_faces=True)

"""A numpy twin of the skeleton-mesh definition, written as loops from the definition, and a PLY reader of
the tests' own (not `meshes.read_ply`).  The rotation of a generic bone is the reference's `rotation_matrix_from_vectors`
verbatim, `(1 - c) / s**2` and all (utils/pose_visualization_utils.py:14-26)."""
import numpy as np

LINES = [(0, 1), (0, 4), (1, 2), (2, 3), (4, 5), (5, 6), (1, 7), (4, 11), (7, 8), (8, 9), (9, 10), (11, 12), (12, 13), (13, 14), (7, 11)]
SPHERE_RADIUS, CYLINDER_RADIUS = 0.02, 0.005
SPHERE_RGB, CYLINDER_RGB = (26, 26, 179), (26, 230, 26)
SPHERE_V, SPHERE_T, CYLINDER_V, CYLINDER_T = 762, 1520, 102, 200
N_VERTICES, N_TRIANGLES = 15 * SPHERE_V + 15 * CYLINDER_V, 15 * SPHERE_T + 15 * CYLINDER_T
HEADER = (b"ply\nformat binary_little_endian 1.0\ncomment Created by Open3D\nelement vertex 12960\nproperty double x\n"
          b"property double y\nproperty double z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n"
          b"element face 25800\nproperty list uchar uint vertex_indices\nend_header\n")


def unit_sphere():
    v = np.zeros((SPHERE_V, 3))
    v[0], v[1] = (0, 0, 1), (0, 0, -1)
    for i in range(1, 20):
        for j in range(40):
            v[2 + 40 * (i - 1) + j] = (np.sin(i * np.pi / 20) * np.cos(j * np.pi / 20), np.sin(i * np.pi / 20) * np.sin(j * np.pi / 20),
                                       np.cos(i * np.pi / 20))
    t = []
    for j in range(40):
        j1 = (j + 1) % 40
        t.append((0, 2 + j, 2 + j1))
        t.append((1, 2 + 40 * 18 + j1, 2 + 40 * 18 + j))
    for i in range(1, 19):
        b1 = 2 + 40 * (i - 1)
        b2 = b1 + 40
        for j in range(40):
            j1 = (j + 1) % 40
            t.append((b2 + j, b1 + j1, b1 + j))
            t.append((b2 + j, b2 + j1, b1 + j1))
    return v, np.array(t, dtype=np.int64)


def cylinder(r, h):
    v = np.zeros((CYLINDER_V, 3))
    v[0], v[1] = (0, 0, h / 2), (0, 0, -h / 2)
    for i in range(5):
        for j in range(20):
            v[2 + 20 * i + j] = (r * np.cos(j * 2 * np.pi / 20), r * np.sin(j * 2 * np.pi / 20), h / 2 - i * h / 4)
    t = []
    for j in range(20):
        j1 = (j + 1) % 20
        t.append((0, 2 + j, 2 + j1))
        t.append((1, 82 + j1, 82 + j))
    for i in range(4):
        b1 = 2 + 20 * i
        b2 = b1 + 20
        for j in range(20):
            j1 = (j + 1) % 20
            t.append((b2 + j, b1 + j1, b1 + j))
            t.append((b2 + j, b2 + j1, b1 + j1))
    return v, np.array(t, dtype=np.int64)


def reference_rotation(vec1, vec2):
    """rotation_matrix_from_vectors, verbatim."""
    a, b = (vec1 / np.linalg.norm(vec1)).reshape(3), (vec2 / np.linalg.norm(vec2)).reshape(3)
    v = np.cross(a, b)
    c = np.dot(a, b)
    s = np.linalg.norm(v)
    kmat = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
    rotation_matrix = np.eye(3) + kmat + kmat.dot(kmat) * ((1 - c) / (s ** 2))
    return rotation_matrix


def bone_rotation(start, end):
    """The rotation of the cylinder between two joints: the reference's where it is defined and well away from the axis, the
    definition's `I + K + K K / (1 + c)` near +z (the same matrix, without the 0 / 0), and the two defined corners."""
    d = end - start
    h = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    if h == 0:
        return np.eye(3)
    b = d / h
    if 1 + b[2] <= 2.0 ** -40:
        return np.diag([1.0, -1.0, -1.0])
    if np.isfinite(b).all() and np.hypot(b[0], b[1]) > 0.05:          # beyond 0.05 rad from +-z
        return reference_rotation(np.array([0.0, 0.0, 1.0]), d)
    v = np.cross([0.0, 0.0, 1.0], b)
    K = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
    return np.eye(3) + K + K @ K / (1 + b[2])


def frame_mesh(joints, crt=None):
    """One frame: (vertices f64 [12960,3], colours u8 [12960,3], triangles i64 [25800,3]).  crt = (c, R, t): every joint p becomes
    c * (p @ R) + t first."""
    joints = np.asarray(joints, dtype=np.float64)
    if crt is not None:
        c, R, t = crt
        joints = np.stack([c * (p @ np.asarray(R)) + np.asarray(t) for p in joints])
    unit, sph_t = unit_sphere()
    verts, cols, tris, off = [], [], [], 0
    with np.errstate(invalid="ignore", divide="ignore"):
        for j in range(15):
            verts.append(SPHERE_RADIUS * unit + joints[j])
            cols.append(np.tile(np.array(SPHERE_RGB, dtype=np.uint8), (SPHERE_V, 1)))
            tris.append(sph_t + off)
            off += SPHERE_V
        for a, b in LINES:
            start, end = joints[a], joints[b]
            d = end - start
            h = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
            v, t = cylinder(CYLINDER_RADIUS, h)
            R = bone_rotation(start, end)
            verts.append(np.stack([R @ p for p in v]) + (start + end) / 2)
            cols.append(np.tile(np.array(CYLINDER_RGB, dtype=np.uint8), (CYLINDER_V, 1)))
            tris.append(t + off)
            off += CYLINDER_V
    return np.concatenate(verts), np.concatenate(cols), np.concatenate(tris)


def part_slices():
    """(first vertex, vertex count, first triangle, triangle count) of the 30 parts in file order."""
    out, v, t = [], 0, 0
    for nv, nt in [(SPHERE_V, SPHERE_T)] * 15 + [(CYLINDER_V, CYLINDER_T)] * 15:
        out.append((v, nv, t, nt))
        v, t = v + nv, t + nt
    return out


def parse_vertex_block(block):
    """349 920 bytes -> (vertices f64 [12960,3], colours u8 [12960,3]), record by record."""
    raw = np.frombuffer(bytes(block), dtype=np.uint8).reshape(N_VERTICES, 27)
    return np.ascontiguousarray(raw[:, :24]).view("<f8").reshape(N_VERTICES, 3), raw[:, 24:].copy()


def parse_face_block(block):
    raw = np.frombuffer(bytes(block), dtype=np.uint8).reshape(N_TRIANGLES, 13)
    assert (raw[:, 0] == 3).all()
    return np.ascontiguousarray(raw[:, 1:]).view("<u4").reshape(N_TRIANGLES, 3).astype(np.int64)


def read_ply(path):
    """The tests' own reader: header line by line, then the two blocks by their counts."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0", lines[:2]
    nv = [int(l.split()[2]) for l in lines if l.startswith("element vertex")][0]
    nf = [int(l.split()[2]) for l in lines if l.startswith("element face")][0]
    props = [l for l in lines if l.startswith("property")]
    assert props == ["property double x", "property double y", "property double z", "property uchar red", "property uchar green",
                     "property uchar blue", "property list uchar uint vertex_indices"], props
    assert len(data) == end + 27 * nv + 13 * nf, (len(data), end, nv, nf)
    assert (nv, nf) == (N_VERTICES, N_TRIANGLES)
    v, c = parse_vertex_block(data[end:end + 27 * nv])
    return v, c, parse_face_block(data[end + 27 * nv:])

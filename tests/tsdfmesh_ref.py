"""TEST INFRASTRUCTURE: NumPy mirror of the TSDF mesh (include/mfhip.h "TSDF mesh"), written from that text and from
the triangulation rules of tests/gridmesh_ref.py (whose tables are imported: the orientation there is decided
geometrically, not by the product's flip table).  Bitwise equal to csrc/tsdfmesh.hip: every float64 expression below is
one IEEE operation per element, associated as the header writes it.

``mesh(volume, origin, pitch, min_weight)`` -> dict(vertices float64 [V, 3], faces int32 [F, 3], normals float64
[V, 3], plus what the tests assert on: ``r`` [V], ``owner`` [V, 4] = (i, j, k, direction), ``cell`` [F, 3] = (i, j, k),
``faces_per_cell`` {(i, j, k): n}, ``branches`` = the gradient branches taken).
"""
import numpy as np

from gridmesh_ref import AXES, DIRS, _corners, _triangles  # noqa: F401  (AXES: the walk order, for the tests)

CENTRAL, FORWARD, BACKWARD, NONE = "central", "forward", "backward", "none"


def tet_faces(t, mask):
    """Number of triangles of tetrahedron t with the inside-corner mask (the rules: 1 or 3 inside -> 1, 2 -> 2)."""
    return len(_triangles(t, mask))


def expected_cell_faces(corner_mask):
    """Faces of one observed cell from its 8-bit inside mask (bit = corner code dx * 4 + dy * 2 + dz)."""
    n = 0
    for t in range(6):
        C = _corners(t)
        m = 0
        for i in range(4):
            m |= (corner_mask >> int(C[i, 0] * 4 + C[i, 1] * 2 + C[i, 2]) & 1) << i
        n += tet_faces(t, m)
    return n


def _gradient(F, usable, q, branches):
    """G [n, 3] at the lattice points q [n, 3] = (i, j, k); F, usable indexed [k, j, i]."""
    nz, ny, nx = F.shape
    dims = (nx, ny, nz)
    G = np.zeros((len(q), 3), np.float64)
    Fq = F[q[:, 2], q[:, 1], q[:, 0]]
    for c in range(3):
        e = np.zeros(3, np.int64)
        e[c] = 1
        plus, minus = q + e, q - e
        hp, hm = plus[:, c] < dims[c], minus[:, c] >= 0
        cp, cm = np.where(hp[:, None], plus, q), np.where(hm[:, None], minus, q)
        hp = hp & usable[cp[:, 2], cp[:, 1], cp[:, 0]]
        hm = hm & usable[cm[:, 2], cm[:, 1], cm[:, 0]]
        Fp, Fm = F[cp[:, 2], cp[:, 1], cp[:, 0]], F[cm[:, 2], cm[:, 1], cm[:, 0]]
        with np.errstate(all="ignore"):
            G[:, c] = np.where(hp & hm, (Fp - Fm) / 2.0, np.where(hp, Fp - Fq, np.where(hm, Fq - Fm, 0.0)))
        for name, sel in ((CENTRAL, hp & hm), (FORWARD, hp & ~hm), (BACKWARD, ~hp & hm), (NONE, ~hp & ~hm)):
            if sel.any():
                branches.add(name)
    return G


def mesh(volume, origin, pitch, min_weight=1.0):
    volume = np.asarray(volume, np.float32)
    nz, ny, nx = volume.shape[:3]
    min_weight, pitch = float(min_weight), float(pitch)
    assert min_weight > 0
    origin = np.asarray([float(x) for x in origin], np.float64)
    F = volume[..., 0].astype(np.float64)
    with np.errstate(invalid="ignore"):
        inside = volume[..., 0] <= 0  # [k, j, i]
        observed = volume[..., 1].astype(np.float64) >= min_weight
    cell_obs = np.ones((nz - 1, ny - 1, nx - 1), bool)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                cell_obs &= observed[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]
    # cell_at[k + 1, j + 1, i + 1] = cell (i, j, k) is observed; False for what is not a cell
    cell_at = np.zeros((nz + 1, ny + 1, nx + 1), bool)
    cell_at[1:nz, 1:ny, 1:nx] = cell_obs
    # active[k, j, i, d]: the owned edge of direction d carries a vertex
    active = np.zeros((nz, ny, nx, 7), bool)
    for d, (ex, ey, ez) in enumerate(DIRS):
        differ = np.zeros((nz, ny, nx), bool)
        differ[:nz - ez, :ny - ey, :nx - ex] = inside[:nz - ez, :ny - ey, :nx - ex] != inside[ez:, ey:, ex:]
        near = np.zeros((nz, ny, nx), bool)
        for sz in ((0,) if ez else (0, 1)):
            for sy in ((0,) if ey else (0, 1)):
                for sx in ((0,) if ex else (0, 1)):
                    near |= cell_at[1 - sz:1 - sz + nz, 1 - sy:1 - sy + ny, 1 - sx:1 - sx + nx]
        active[..., d] = differ & near
    vid = (np.cumsum(active.reshape(-1)) - 1).reshape(active.shape)  # rank in (k, j, i, direction) order
    at = np.argwhere(active)  # rows (k, j, i, d), lexicographic
    a = at[:, [2, 1, 0]]
    b = a + np.asarray(DIRS, np.int64)[at[:, 3]]
    Fa, Fb = F[a[:, 2], a[:, 1], a[:, 0]], F[b[:, 2], b[:, 1], b[:, 0]]
    r = Fa / (Fa - Fb)
    pa = origin + pitch * a.astype(np.float64)
    pb = origin + pitch * b.astype(np.float64)
    vertices = pa + r[:, None] * (pb - pa)
    branches = set()
    Ga, Gb = _gradient(F, observed, a, branches), _gradient(F, observed, b, branches)
    g = Ga + r[:, None] * (Gb - Ga)
    s = (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]
    with np.errstate(all="ignore"):
        ok = s > 0.0
        normals = np.where(ok[:, None], g / np.sqrt(s)[:, None], 0.0)
    # faces
    cell = np.argwhere(cell_obs)[:, [2, 1, 0]]  # (i, j, k) of the observed cells
    dir_index = {d: n for n, d in enumerate(DIRS)}
    rows, keys = [], []
    for t in range(6):
        C = _corners(t)  # [4, 3] offsets (dx, dy, dz)
        m = np.zeros(len(cell), np.int64)
        for i in range(4):
            q = cell + C[i]
            m |= inside[q[:, 2], q[:, 1], q[:, 0]].astype(np.int64) << i
        for mask in range(1, 15):
            sel = cell[m == mask]
            if not len(sel):
                continue
            for n, tri in enumerate(_triangles(t, mask)):
                f = []
                for i, j in tri:
                    q, d = sel + C[i], dir_index[tuple(int(x) for x in C[j] - C[i])]
                    assert active[q[:, 2], q[:, 1], q[:, 0], d].all()  # no face names a missing vertex
                    f.append(vid[q[:, 2], q[:, 1], q[:, 0], d])
                rows.append(np.stack(f, 1))
                keys.append(np.concatenate([sel[:, [2, 1, 0]], np.full((len(sel), 1), t), np.full((len(sel), 1), n)], 1))
    if rows:
        rows, keys = np.concatenate(rows), np.concatenate(keys)
        order = np.lexsort(keys.T[::-1])  # (k, j, i, tetrahedron, triangle)
        faces, face_cell = rows[order].astype(np.int32), keys[order][:, [2, 1, 0]]
    else:
        faces, face_cell = np.zeros((0, 3), np.int32), np.zeros((0, 3), np.int64)
    if len(vertices):
        assert len(faces) and np.array_equal(np.unique(faces), np.arange(len(vertices)))  # every vertex is used
    per_cell = {}
    for c in map(tuple, face_cell.tolist()):
        per_cell[c] = per_cell.get(c, 0) + 1
    return dict(vertices=vertices.reshape(-1, 3), faces=faces, normals=normals.reshape(-1, 3), r=r,
                owner=np.concatenate([a, at[:, 3:]], 1), cell=face_cell, faces_per_cell=per_cell, branches=branches)


# ---- properties of a mesh (asserted on the mirror alone) ------------------------------------------------------------
def edge_pairing(faces):
    """-> (closed, n_edges): every undirected edge lies in exactly two faces, once in each direction."""
    f = np.asarray(faces, np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    n = int(f.max()) + 1
    code, rev = e[:, 0] * n + e[:, 1], e[:, 1] * n + e[:, 0]
    closed = (len(np.unique(code)) == len(code) and np.array_equal(np.sort(code), np.sort(rev))
              and bool((e[:, 0] != e[:, 1]).all()))
    return closed, len(np.unique(np.minimum(code, rev)))


def signed_volume(vertices, faces):
    p = np.asarray(vertices, np.float64)[np.asarray(faces, np.int64)]
    return float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)

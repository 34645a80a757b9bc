"""TEST HELPER: NumPy mirror of csrc/gridmesh.hip and of the render-service route built on it -- grid_msg_to_mesh
(ros/src/morefusion_ros/nodes/voxel_grids_to_mesh_markers.py:80-97), the label test of nodes/render_voxel_grids.py:58-99
and OctomapServer::getGridsInWorldFrame (OctomapServer.cpp:456-508).  Written from the issue's definitions and the
reference's Python, not from the kernels; the product is checked against it bit for bit.

Surface: the 0.5-level set of the occupancy (value > 0) over the six-tetrahedra (Kuhn) subdivision of the grid padded
by one empty layer (trimesh / scikit-image parity unpinned, DESIGN.md "Grid meshes").

Order.  A lattice point owns the edges towards DIRS, in that order; an edge whose ends differ in occupancy is a vertex,
numbered by its rank in (padded x, y, z, direction) order; position = origin + pitch * ((pa + pb) / 2 - 1), float64.
Tetrahedron t = 0..5 of a cell walks the axes AXES[t] = xyz, xzy, yxz, yzx, zxy, zyx: corners c0 = cell, c1 = c0 + e_a,
c2 = c1 + e_b, c3 = cell + (1,1,1).  With e(i,j) the vertex on the edge between corners i and j:
  * one corner i alone on its side:  (e(i,j0), e(i,j1), e(i,j2)) with j ascending;
  * corners a < b occupied, c < d empty:  (e(a,c), e(a,d), e(b,d)), then (e(a,c), e(b,d), e(b,c)).
A triangle's last two vertices are exchanged where that makes it counter-clockwise seen from the empty side; here that
is decided geometrically (the normal against the direction from the occupied corners to the empty ones), not by a table.
Faces are numbered in (cell x, y, z, tetrahedron, triangle) order.

Humphrey filter as the issue recalls trimesh's (unpinned): q = v; v = L q; b = v - (alpha v0 + (1 - alpha) q);
v = v - (beta b + (1 - beta) L b); L x = mean of x over the heads of the directed half-edges leaving the vertex, summed
in ascending vertex index, float64.
"""
import numpy as np

import render_ref

DIRS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))
AXES = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))


def _corners(t):
    c = np.zeros((4, 3), np.int64)
    c[1, AXES[t][0]] = 1
    c[2] = c[1]
    c[2, AXES[t][1]] = 1
    c[3] = 1
    return c


def _triangles(t, mask):
    """The triangles of tetrahedron t with the occupied-corner mask, as corner pairs (i, j), i < j, oriented."""
    inside = [i for i in range(4) if mask >> i & 1]
    outside = [i for i in range(4) if not mask >> i & 1]
    if not inside or not outside:
        return []
    pair = lambda i, j: (min(i, j), max(i, j))  # noqa: E731
    if len(inside) == 2:
        (a, b), (c, d) = inside, outside
        tris = [[pair(a, c), pair(a, d), pair(b, d)], [pair(a, c), pair(b, d), pair(b, c)]]
    else:
        i = inside[0] if len(inside) == 1 else outside[0]
        tris = [[pair(i, j) for j in range(4) if j != i]]
    P = _corners(t).astype(np.float64)
    towards_empty = P[outside].mean(axis=0) - P[inside].mean(axis=0)
    out = []
    for tri in tris:
        m = [(P[i] + P[j]) / 2 for i, j in tri]
        n = np.cross(m[1] - m[0], m[2] - m[0])
        s = float(n @ towards_empty)
        assert abs(s) > 1e-9
        out.append(tri if s > 0 else [tri[0], tri[2], tri[1]])
    return out


def mesh(grid, pitch, origin, return_cases=False):
    """One grid [X, Y, Z] -> (vertices float64 [V, 3], faces int32 [F, 3]) (and the [6, 16] histogram of the cases)."""
    occ = np.pad(np.asarray(grid) > 0, 1)
    P = occ.shape
    ext = np.pad(occ, ((0, 1), (0, 1), (0, 1)))
    active = np.stack([occ != ext[d[0]:d[0] + P[0], d[1]:d[1] + P[1], d[2]:d[2] + P[2]] for d in DIRS], axis=-1)
    vid = (np.cumsum(active.reshape(-1)) - 1).reshape(active.shape)
    pa = np.argwhere(active)  # rows (x, y, z, direction) in lexicographic order
    pb = pa[:, :3] + np.asarray(DIRS)[pa[:, 3]]
    vertices = np.asarray(origin, np.float64) + np.float64(pitch) * ((pa[:, :3] + pb).astype(np.float64) / 2 - 1)
    cx, cy, cz = np.meshgrid(*(np.arange(n - 1) for n in P), indexing="ij")
    cell = np.stack([cx, cy, cz], -1).reshape(-1, 3)
    dir_index = {d: k for k, d in enumerate(DIRS)}
    rows, keys = [], []
    cases = np.zeros((6, 16), np.int64)
    for t in range(6):
        C = _corners(t)
        m = np.zeros(len(cell), np.int64)
        for i in range(4):
            q = cell + C[i]
            m |= occ[q[:, 0], q[:, 1], q[:, 2]].astype(np.int64) << i
        cases[t] = np.bincount(m, minlength=16)
        for mask in range(1, 15):
            sel = cell[m == mask]
            if not len(sel):
                continue
            for k, tri in enumerate(_triangles(t, mask)):
                f = []
                for i, j in tri:
                    q = sel + C[i]
                    f.append(vid[q[:, 0], q[:, 1], q[:, 2], dir_index[tuple(C[j] - C[i])]])
                    assert active[q[:, 0], q[:, 1], q[:, 2], dir_index[tuple(C[j] - C[i])]].all()
                rows.append(np.stack(f, 1))
                keys.append(np.concatenate([sel, np.full((len(sel), 1), t), np.full((len(sel), 1), k)], 1))
    if rows:
        rows, keys = np.concatenate(rows), np.concatenate(keys)
        order = np.lexsort(keys.T[::-1])
        faces = rows[order].astype(np.int32)
    else:
        faces = np.zeros((0, 3), np.int32)
    out = (vertices.reshape(-1, 3), faces)
    return out + (cases,) if return_cases else out


def neighbours(faces, n_vertices):
    """(rows int64 [V, max degree] padded with -1, degree [V]): row a = the sorted heads of the half-edges a -> b."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    tail = np.concatenate([f[:, 0], f[:, 1], f[:, 2]])
    head = np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
    order = np.lexsort((head, tail))
    tail, head = tail[order], head[order]
    deg = np.bincount(tail, minlength=n_vertices)
    start = np.concatenate([[0], np.cumsum(deg)])
    rows = np.full((n_vertices, max(int(deg.max()) if n_vertices else 0, 1)), -1, np.int64)
    rows[tail, np.arange(len(tail)) - start[tail]] = head
    return rows, deg


def _laplacian(x, rows, deg):
    s = np.zeros_like(x)
    for k in range(rows.shape[1]):
        s = np.where((k < deg)[:, None], s + x[np.maximum(rows[:, k], 0)], s)
    return s / deg[:, None].astype(np.float64)


def humphrey(vertices, faces, alpha=0.1, beta=0.5, iterations=10):
    v0 = np.asarray(vertices, np.float64).reshape(-1, 3)
    if not len(v0) or iterations == 0:
        return v0.copy()
    rows, deg = neighbours(faces, len(v0))
    assert deg.min() >= 1
    alpha, beta = np.float64(alpha), np.float64(beta)
    v = v0.copy()
    for _ in range(iterations):
        q = v
        v = _laplacian(q, rows, deg)
        b = v - (alpha * v0 + (np.float64(1.0) - alpha) * q)
        v = v - (beta * b + (np.float64(1.0) - beta) * _laplacian(b, rows, deg))
    return v


def voxel_grids_to_meshes(grids, pitch, origin, smooth=True, alpha=0.1, beta=0.5, iterations=10):
    out = []
    for g, h, o in zip(grids, pitch, origin):
        v, f = mesh(g, h, o)
        out.append((humphrey(v, f, alpha, beta, iterations) if smooth else v, f))
    return out


# ---- properties of a mesh (asserted on the mirror alone) ----------------------------------------------------------
def half_edges_closed(faces):
    """Every directed half-edge occurs exactly once and its reverse exactly once."""
    f = np.asarray(faces, np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    code = e[:, 0] * (f.max() + 1) + e[:, 1]
    rev = e[:, 1] * (f.max() + 1) + e[:, 0]
    return len(np.unique(code)) == len(code) and np.array_equal(np.sort(code), np.sort(rev)) and (e[:, 0] != e[:, 1]).all()


def components(faces, n_vertices):
    """Number of connected components of the surface (union-find over the edges)."""
    parent = np.arange(n_vertices)

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    f = np.asarray(faces, np.int64)
    for a, b in np.concatenate([f[:, [0, 1]], f[:, [1, 2]]]):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[ra] = rb
    return len({find(a) for a in range(n_vertices)})


def euler(faces, n_vertices):
    f = np.asarray(faces, np.int64)
    return n_vertices - 3 * len(f) // 2 + len(f)  # closed: every edge has two half-edges


def volume(vertices, faces):
    p = np.asarray(vertices, np.float64)[np.asarray(faces, np.int64)]
    return float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)


def surface_cells(grid):
    """Lattice cells (of the padded grid) whose 8 corners are neither all occupied nor all empty."""
    occ = np.pad(np.asarray(grid) > 0, 1).astype(np.int64)
    n = sum(occ[a:occ.shape[0] - 1 + a, b:occ.shape[1] - 1 + b, c:occ.shape[2] - 1 + c]
            for a in (0, 1) for b in (0, 1) for c in (0, 1))
    return int(((n > 0) & (n < 8)).sum())


# ---- the render service ------------------------------------------------------------------------------------------
def label_of_render(depth_rendered, instance, depth_sensor):
    """render_voxel_grids.py:66-99 -> (label int32 [H, W], the number of pixels each branch changes)."""
    label = np.full(instance.shape, -2, np.int32)
    drawn = instance != -1
    label[drawn] = instance[drawn]
    with np.errstate(invalid="ignore"):
        behind = drawn & (depth_rendered > (depth_sensor + np.float32(0.01)))
    label[behind] = -2
    counts = dict(drawn=int(drawn.sum()), behind=int(behind.sum()), nan_kept=int((drawn & np.isnan(depth_sensor)).sum()))
    return label, counts


def render_voxel_grids(grids, depth, K, T_sensor_to_map, height, width, return_parts=False):
    meshes = voxel_grids_to_meshes(grids["grid"], grids["pitch"], grids["origin"])
    keep = [i for i, (v, f) in enumerate(meshes) if len(f)]
    if not keep:
        label, counts = np.full((height, width), -2, np.int32), {}
        return (label, counts, None) if return_parts else label
    T = np.linalg.inv(np.asarray(T_sensor_to_map, np.float64))
    out = render_ref.render([meshes[i] for i in keep], [T] * len(keep), K, height, width,
                            instance_ids=[grids["instance_ids"][i] for i in keep])
    label, counts = label_of_render(out["depth"][0], out["instance"][0], np.asarray(depth, np.float32))
    return (label, counts, out) if return_parts else label


def grids_in_map_frame(ref_server, dim=32):
    """getGridsInWorldFrame over tests/occserver_ref.OctomapServer (background id 0, tracked ids >= 1)."""
    import occmap_ref as R
    import occtrack_ref as T
    ids = [i for i in sorted(ref_server.octrees) if i != 0 and i in ref_server.centers]
    B = len(ids)
    out = dict(instance_ids=ids, class_ids=[ref_server.class_ids[i] for i in ids], pitch=np.zeros(B, np.float32),
               origin=np.zeros((B, 3), np.float64), grid=np.zeros((B, dim, dim, dim), np.float32))
    index = np.argwhere(np.ones((dim, dim, dim), bool))
    for b, iid in enumerate(ids):
        tree = ref_server.octrees[iid]
        p32 = np.float32(tree.resolution)
        origin = ref_server.centers[iid].astype(np.float64) - (dim / 2.0 - 0.5) * np.float64(p32)
        x = origin + (p32 * index.astype(np.float32)).astype(np.float64)
        s = np.floor(x * tree.res_factor)
        ok = ((s >= -R.KEY_MAX) & (s < R.KEY_MAX)).all(axis=1)
        l = T._Table(tree)(np.where(ok[:, None], s, 0).astype(np.int64) + R.KEY_MAX)
        l[~ok] = np.nan
        g = np.zeros(len(index), np.float32)
        for at in np.flatnonzero(~np.isnan(l)):
            occ = R.probability(l[at])
            if occ > 0.5:
                g[at] = np.float32(occ)
        out["pitch"][b], out["origin"][b], out["grid"][b] = p32, origin, g.reshape(dim, dim, dim)
    return out

"""TEST INFRASTRUCTURE: the sparse conv3 of the bf16 training path (csrc/sparseconv_bf16.hip + the compact-row forms
of k_avgvox_cl_fwd / _bwd in csrc/voxelize.hip), STAGE BY STAGE through the C ABI, shared by the emulator tests (CPU
tensors as device memory) and tests/test_gpu_sparseconv_bf16.py (the MI355X).

The ten kernels around the two MFMA engines are indexing plus short fp32 sums in a documented order ("increasing point
index", "tap order", "slot order"); the library is built with -ffp-contract=off, IEEE divide and round-to-nearest-even
bf16 conversion.  So every stage has an EXACT reference: integers for the tables, bit patterns for the values.  The
references below are plain numpy; every case feeds ONE stage with the reference's tables and tensors (not with the
previous kernel's output) and compares every element for equality.  Values are drawn so that no sum or quotient is
denormal or overflows (``rand_bits``): the device's denormal mode is no factor.

``wiring_case`` (the operator end to end) is the one place with a tolerance: a float64 dense convolution over the
reference's bf16 mean rows, per element under the bounds derived in its docstring."""
import ctypes

import numpy as np
import torch
import torch.nn.functional as F

import bf16_bound as BB

BF = torch.bfloat16
SENT = -9.0                # sentinel of memory a kernel must leave alone (exact in bf16)
SENT_BITS = 0xC110         # ... its bf16 bit pattern
NAN_BITS = 0x7FC1          # a bf16 NaN: rows nothing may read
WIDE = dict(emin=-20, emax=6)
KPAD = 128                 # rows a class is padded to (sparseconv_bf16.hip: kPadRows)
GEOM = (4, 2, 1, 1)        # conv3: kernel 4, stride 2, pad 1


def p(t):
    return None if t is None or t.numel() == 0 else t.data_ptr()


def ok(code, L=None):
    assert code == 0, (code, L.mf_last_error_string().decode() if L is not None and hasattr(L, "mf_last_error_string") else "")


# ------------------------------------------------------------------------------------------------- bf16 bit patterns
def bf16_bits(x):
    """float32 array -> uint16 bf16 bit patterns, round to nearest even (finite values)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_f32(bits):
    """uint16 bf16 bit patterns -> float32 (exact)."""
    return (np.ascontiguousarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def to_t(bits, dev):
    """uint16 bit patterns -> torch bf16 tensor on ``dev``."""
    return torch.from_numpy(np.ascontiguousarray(bits, np.uint16).view(np.int16).copy()).view(BF).to(dev)


def to_bits(t):
    """torch bf16 tensor -> uint16 bit patterns on the host."""
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16).copy()


def rand_bits(rs, *shape, zeros=0.1, emin=-6, emax=1):
    """Random bf16 bit patterns: magnitude (1 + m / 128) 2^e, e in [emin, emax], random sign, a tenth exact zeros.
    [2^-6, 4) by default; the operands of a SUM take WIDE (27 binades): over a few binades the fp32 sums of 8-bit
    significands are exact, and an accumulator of another precision or order would give the same bits.  The smallest
    non-zero partial sum is then 2^-27, a quotient by a count 2^-34: no denormals."""
    e = rs.randint(emin, emax + 1, shape) + 127
    m = rs.randint(0, 128, shape)
    s = rs.randint(0, 2, shape)
    bits = ((s << 15) | (e << 7) | m).astype(np.uint16)
    bits[rs.uniform(size=shape) < zeros] = 0
    return bits


def rand_f32(rs, *shape):
    """fp32 values of magnitude [2^-6, 4), all 24 bits random (a bias, a dense pre-activation, a weight), among them
    ties of the bf16 rounding on even and odd last bits."""
    hi = rand_bits(rs, *shape, zeros=0.0).astype(np.uint32) << 16
    lo = rs.randint(0, 1 << 16, shape).astype(np.uint32)
    lo[rs.uniform(size=shape) < 0.05] = 0x8000
    return (hi | lo).view(np.float32)


def same(got, ref, what):
    """Every element equal (bit patterns / integers); names the first few that are not."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if not np.array_equal(got, ref):
        bad = np.argwhere(got != ref)
        first = [(tuple(int(v) for v in i), got[tuple(i)].item(), ref[tuple(i)].item()) for i in bad[:5]]
        raise AssertionError(f"{what}: {len(bad)} of {got.size} elements differ; (index, got, want): {first}")


# -------------------------------------------------------------------------------------------------------- the tables
def voxel_keys(pts, bi, B, D):
    """key = b D^3 + (rx D + ry) D + rz of every point, -1 outside.  r = round half AWAY from zero (roundf), in
    float32; NaN compares false: outside."""
    x = np.asarray(pts, np.float32)
    with np.errstate(invalid="ignore"):
        r = np.sign(x) * np.floor(np.abs(x) + np.float32(0.5))
        inside = ((r >= 0) & (r < np.float32(D))).all(1) & (bi >= 0) & (bi < B)
    ri = np.where(inside[:, None], r, 0).astype(np.int64)
    key = bi.astype(np.int64) * D ** 3 + (ri[:, 0] * D + ri[:, 1]) * D + ri[:, 2]
    return np.where(inside, key, -1)


def max_rows(n):
    """scb_max_rows restated: every class may waste up to 127 pad rows."""
    return -(-(n + 8 * (KPAD - 1)) // KPAD) * KPAD


def voxel_class(key, D):
    v = key % D ** 3
    ix, iy, iz = v // (D * D), (v // D) % D, v % D
    return ((ix + 1) & 1) | (((iy + 1) & 1) << 1) | (((iz + 1) & 1) << 2)


def tables_ref(pts, bi, B, D, chain_seed=None):
    """The tables of mf_sparse_conv3_bf16_index.  ``chain_seed``: also head / link with every chain in a RANDOM order
    (the atomics fix only the members of a chain; a kernel that reads the chains must sort them itself)."""
    n, BV, Mp = len(pts), B * D ** 3, max_rows(len(pts))
    key = voxel_keys(pts, bi, B, D)
    counts = np.bincount(key[key >= 0], minlength=BV).astype(np.int32)
    occ = np.flatnonzero(counts > 0)
    cls = voxel_class(occ, D)
    class_off = np.zeros(9, np.int32)
    rowmap = np.full(BV, -1, np.int32)
    rowvox = np.full(Mp, -1, np.int32)
    off = 0
    for c in range(8):
        class_off[c] = off
        mine = occ[cls == c]                              # increasing b D^3 + v
        rowmap[mine] = off + np.arange(len(mine))
        rowvox[off:off + len(mine)] = mine
        off += -(-len(mine) // KPAD) * KPAD
    class_off[8] = off
    assert off <= Mp
    tile_group = np.full(Mp // 64, -1, np.int32)
    for c in range(8):
        tile_group[class_off[c] // 64:class_off[c + 1] // 64] = c
    T = dict(n=n, B=B, D=D, Mp=Mp, key=key, counts=counts, rowmap=rowmap, rowvox=rowvox, class_off=class_off,
             tile_group=tile_group)
    if chain_seed is not None:
        rs = np.random.RandomState(chain_seed)
        head = np.full(BV, -1, np.int32)
        link = np.full(max(n, 1), -2, np.int32)
        order = np.argsort(key, kind="stable")
        order = order[key[order] >= 0]
        for k, grp in zip(*_groups(key[order], order)):
            grp = rs.permutation(grp)
            if len(grp) > 1 and np.all(np.diff(grp) > 0):   # never the sorted order by luck
                grp = grp[::-1]
            head[k] = grp[0]
            link[grp[:-1]] = grp[1:]
            link[grp[-1]] = -1
        T.update(head=head, link=link)
    return T


def _groups(sorted_keys, idx):
    """-> (distinct keys, the index groups of each) of an array sorted by key."""
    if len(sorted_keys) == 0:
        return [], []
    cut = np.flatnonzero(np.diff(sorted_keys)) + 1
    return sorted_keys[np.r_[0, cut]], np.split(idx, cut)


class Workspace:
    """The index workspace on ``dev`` with the tables' places in it (mf_sparse_conv3_bf16_tables): read a table back,
    or put the reference's there."""
    NAMES = ("tile_group", "class_off", "rowmap", "counts", "rowvox", "head", "link")

    def __init__(self, L, dev, n, B, D, fill=0xA5):
        nbytes = int(L.mf_sparse_conv3_bf16_workspace_bytes(n, B, D))
        assert nbytes > 0
        assert int(L.mf_sparse_conv3_bf16_max_rows(n)) == max_rows(n)
        self.t = torch.full((nbytes,), fill, dtype=torch.uint8, device=dev)   # (stale bytes: the index fills what it needs)
        tabs = (ctypes.c_int64 * 7)()
        ok(L.mf_sparse_conv3_bf16_tables(self.t.data_ptr(), n, B, D, tabs), L)
        BV, Mp = B * D ** 3, max_rows(n)
        sizes = dict(tile_group=Mp // 64, class_off=9, rowmap=BV, counts=BV, rowvox=Mp, head=BV, link=max(n, 1))
        self.where = {}
        for name, addr in zip(self.NAMES, tabs):
            off = int(addr) - self.t.data_ptr()
            assert 0 <= off and off % 256 == 0 and off + 4 * sizes[name] <= nbytes, (name, off, nbytes)
            self.where[name] = (off, sizes[name])
        spans = sorted(self.where.values())
        assert all(a + 4 * na <= b for (a, na), (b, _) in zip(spans, spans[1:])), "tables overlap"

    def ptr(self):
        return self.t.data_ptr()

    def read(self, name):
        off, cnt = self.where[name]
        return self.t[off:off + 4 * cnt].cpu().numpy().view(np.int32).copy()

    def write(self, name, a):
        off, cnt = self.where[name]
        a = np.ascontiguousarray(a, np.int32)
        assert a.shape == (cnt,), (name, a.shape, cnt)
        self.t[off:off + 4 * cnt] = torch.from_numpy(a.view(np.uint8).copy()).to(self.t.device)

    def put(self, T, names=("tile_group", "class_off", "rowmap", "counts", "rowvox")):
        for name in names:
            self.write(name, T[name])
        return self


# -------------------------------------------------------------------------------------------------------- the points
def points_faces(B, D, n=150, seed=11, piles=()):
    """Case 1's points: random ones over the grid and a little beyond its faces, coordinates exactly on .5 (2.5 -> 3
    and 0.5 -> 1: half away from zero, not to even; -0.5 -> -1 and D - 0.5 -> D: outside), -0.4 (-> -0: inside), a
    NaN row, batch indices -1 and B, several points in one voxel.  ``piles``: further voxels with that many points."""
    rs = np.random.RandomState(seed)
    pts = rs.uniform(-0.45, D - 0.55, (n, 3)).astype(np.float32)
    bi = rs.randint(0, B, n).astype(np.int32)
    pts[:8] = rs.uniform(-2.0, D + 1.0, (8, 3))
    pts[8] = (2.5, 1.0, 1.0)
    pts[9] = (-0.5, 1.0, 1.0)
    pts[10] = (D - 0.5, 1.0, 1.0)
    pts[11] = (-0.4, 0.3, 2.0)
    pts[12] = (1.0, np.nan, 1.0)
    pts[13] = (0.5, 1.5, 4.5)
    pts[14] = (1.0, D - 0.5, 1.0)
    pts[15] = (1.0, 1.0, -0.5)
    pts[16] = (D - 1.0, D - 0.6, D - 1.4)       # the far corner voxel
    pts[17] = (0.0, 0.0, 0.0)
    bi[18], bi[19] = -1, B
    pts[20:26] = np.asarray((3.2, 4.1, 2.9), np.float32) + rs.uniform(-0.2, 0.2, (6, 3))
    bi[20:26] = B - 1
    extra_p, extra_b = [], []
    for j, cnt in enumerate(piles):
        centre = np.asarray(((1 + 2 * j) % D, (2 + j) % D, (4 + j) % D), np.float32)
        mine = (np.round(pts) == centre).all(1) & (bi == j % B)
        pts[mine] = (0.1, 0.2, -0.1)            # (the pile has exactly ``cnt`` points: the others move to the corner)
        extra_p.append(centre + rs.uniform(-0.3, 0.3, (cnt, 3)))
        extra_b.append(np.full(cnt, j % B, np.int32))
    if piles:
        pts = np.concatenate([pts] + extra_p).astype(np.float32)
        bi = np.concatenate([bi] + extra_b)
        perm = rs.permutation(len(pts))     # pile members scattered over the point index
        pts, bi = pts[perm], bi[perm]
    return np.ascontiguousarray(pts, np.float32), np.ascontiguousarray(bi, np.int32)


def points_of_voxels(keys, D, rs, extra=40):
    """One point inside each voxel of ``keys`` (b D^3 + v), ``extra`` more in voxels already taken, shuffled."""
    keys = np.concatenate((keys, rs.choice(keys, extra)))
    keys = keys[rs.permutation(len(keys))]
    v = keys % D ** 3
    centre = np.stack((v // (D * D), (v // D) % D, v % D), 1).astype(np.float32)
    pts = centre + rs.uniform(-0.3, 0.3, centre.shape).astype(np.float32)
    return np.ascontiguousarray(pts, np.float32), np.ascontiguousarray(keys // D ** 3, np.int32)


PAD_CLASS_COUNTS = (128, 129, 1, 0, 37, 127, 256, 3)


def points_class_padding(seed=12):
    """Case 2: B = 3, D = 16 (6 index workgroups); occupied voxels per class = PAD_CLASS_COUNTS: exactly 128 (the next
    class starts at + 128), 129 (+ 256), 1, none."""
    B, D = 3, 16
    rs = np.random.RandomState(seed)
    allk = np.arange(B * D ** 3)
    cls = voxel_class(allk, D)
    keys = np.concatenate([rs.choice(allk[cls == c], m, replace=False) for c, m in enumerate(PAD_CLASS_COUNTS)])
    pts, bi = points_of_voxels(keys, D, rs)
    return pts, bi, B, D


def points_prefix_carry(seed=13):
    """Case 3: B = 3, D = 32: 48 index workgroups, scanned in chunks of 32 with a carry; ~3000 points."""
    B, D = 3, 32
    rs = np.random.RandomState(seed)
    pts = rs.uniform(-0.45, D - 0.55, (3000, 3)).astype(np.float32)
    bi = rs.randint(0, B, 3000).astype(np.int32)
    return pts, bi, B, D


# ------------------------------------------------------------------------------------------------ case 1 - 3: index
def index_case(L, dev, st, pts, bi, B, D, what):
    """mf_sparse_conv3_bf16_index: EVERY table element equal to the reference; the chains as sets."""
    n = len(pts)
    T = tables_ref(pts, bi, B, D)
    ws = Workspace(L, dev, n, B, D)
    pd = torch.from_numpy(pts).to(dev) if n else None
    bd = torch.from_numpy(bi).to(dev) if n else None
    ok(L.mf_sparse_conv3_bf16_index(p(pd), p(bd), n, B, D, ws.ptr(), st()), L)
    for name in ("counts", "class_off", "rowmap", "rowvox", "tile_group"):
        same(ws.read(name), T[name], f"{what} {name}")
    head, link = ws.read("head"), ws.read("link")
    key = T["key"]
    if n:
        same(link[key < 0], np.full(int((key < 0).sum()), -2, np.int32), f"{what} link of points outside")
    same(head[T["counts"] == 0], np.full(int((T["counts"] == 0).sum()), -1, np.int32), f"{what} head of empty voxels")
    order = np.argsort(key, kind="stable")
    order = order[key[order] >= 0]
    for k, grp in zip(*_groups(key[order], order)):
        walk, m = [], int(head[k])
        for _ in range(int(T["counts"][k])):
            assert 0 <= m < n, f"{what}: chain of voxel {k} leaves the points at {m}"
            walk.append(m)
            m = int(link[m])
        assert m == -1, f"{what}: chain of voxel {k} does not end after its count"
        assert sorted(walk) == sorted(int(i) for i in grp), f"{what}: chain of voxel {k}: {walk} != {list(grp)}"
    return T


def index_empty_case(L, dev, st, B, D):
    """n = 0: no voxel has a row, every class offset is 0, no block has a class."""
    T = index_case(L, dev, st, np.zeros((0, 3), np.float32), np.zeros(0, np.int32), B, D, f"index n=0 B{B} D{D}")
    assert (T["rowmap"] == -1).all() and (T["class_off"] == 0).all() and (T["tile_group"] == -1).all()


def assert_faces_cover(T, pts, bi, B, D):
    """The points of case 1 reach what they are for."""
    key = T["key"]
    kof = lambda i: int(key[i])
    assert kof(8) == bi[8] * D ** 3 + (3 * D + 1) * D + 1           # 2.5 -> 3
    assert kof(9) == -1 and kof(10) == -1 and kof(14) == -1 and kof(15) == -1
    assert kof(11) == bi[11] * D ** 3 + 2                            # -0.4 -> -0: voxel (0, 0, 2)
    assert kof(12) == -1 and kof(18) == -1 and kof(19) == -1
    assert kof(13) == bi[13] * D ** 3 + (1 * D + 2) * D + 5          # 0.5 -> 1, 1.5 -> 2, 4.5 -> 5
    assert kof(16) == bi[16] * D ** 3 + D ** 3 - 1
    assert int(T["counts"].max()) >= 6


def assert_padding_covers(T):
    co, cnt = T["class_off"], PAD_CLASS_COUNTS
    per = [int(((T["rowvox"][co[c]:co[c + 1]]) >= 0).sum()) for c in range(8)]
    assert tuple(per) == cnt, per
    assert co[1] - co[0] == 128 and co[2] - co[1] == 256 and co[3] - co[2] == 128 and co[4] == co[3]


def assert_carry_covers(T, D):
    occ = np.flatnonzero(T["counts"] > 0)
    cls = voxel_class(occ, D)
    for c in range(8):
        assert ((occ < 65536) & (cls == c)).any() and ((occ >= 65536) & (cls == c)).any(), c
    assert -(-len(T["counts"]) // 2048) == 48


# --------------------------------------------------------------------------------------------- case 4: the mean rows
def mean_rows_ref(vbits, T, C):
    """-> {key: bf16 bits [C]} of every occupied voxel: fp32 sum of its points' rows in increasing point index, one
    add at a time, divided by float32(count), rounded to bf16."""
    key = T["key"]
    order = np.argsort(key, kind="stable")      # stable: increasing point index inside a key
    order = order[key[order] >= 0]
    vals = bf16_f32(vbits[:, :C])
    out = {}
    for k, grp in zip(*_groups(key[order], order)):
        s = np.zeros(C, np.float32)
        for i in grp:
            s = s + vals[i]
        out[int(k)] = bf16_bits(s / np.float32(len(grp)))
    return out


def grad_rows_ref(gbits, rows, T, C):
    """gvalues[i, :C] = bf16(float32(g[rows[key_i], c]) / float32(count)); zero rows for points outside."""
    key = T["key"]
    out = np.zeros((T["n"], C), np.uint16)
    inside = key >= 0
    g = bf16_f32(gbits[rows[key[inside]], :C])
    out[inside] = bf16_bits(g / T["counts"][key[inside]].astype(np.float32)[:, None])
    return out


def cancel_pairs(rs, vbits, T, C):
    """Two points of every voxel with >= 3 get + X and - X, X in [2^10, 2^16), the others values below 2^-7: the
    fp32 sum of the voxel then depends on WHERE the small rows stand between the two (x + X - X loses x next to X,
    X - X + x keeps it), so a sum taken in another order than increasing point index differs in the leading bits, not
    in the last ulp that the bf16 rounding of the mean would hide."""
    key = T["key"]
    order = np.argsort(key, kind="stable")
    order = order[key[order] >= 0]
    for _, grp in zip(*_groups(key[order], order)):
        if len(grp) >= 3:
            a, b = rs.choice(grp, 2, replace=False)
            vbits[grp, :C] = rand_bits(rs, len(grp), C, emin=-20, emax=-8)
            X = rand_bits(rs, C, zeros=0.0, emin=10, emax=15)
            vbits[a, :C], vbits[b, :C] = X, X ^ 0x8000


def mean_rows_case(L, dev, st, pts, bi, B, D, C, seed=21, what="mean rows"):
    """mf_average_voxelization_rows_bf16_fwd / _bwd on the REFERENCE's tables (chains in a random order), row pitches
    beyond the data; then the dense form mf_average_voxelization_cl_bf16_fwd / _bwd, which links its own chains."""
    rs = np.random.RandomState(seed)
    n = len(pts)
    T = tables_ref(pts, bi, B, D, chain_seed=seed)
    assert int(T["counts"].max()) == 70 and int(np.sort(T["counts"])[-2]) == 64, "one voxel on each side of cnt <= 64"
    Mp, BV = T["Mp"], B * D ** 3
    ldv, lda, ldg, ldx = C + 6, C + 2, C + 4, C + 8
    vbits = rand_bits(rs, n, ldv, **WIDE)
    vbits[:, C:] = NAN_BITS                      # beyond the C columns: never read
    cancel_pairs(rs, vbits, T, C)
    means = mean_rows_ref(vbits, T, C)
    pd, bd, vd = torch.from_numpy(pts).to(dev), torch.from_numpy(bi).to(dev), to_t(vbits, dev)
    tab = {k: torch.from_numpy(T[k]).to(dev) for k in ("counts", "head", "link", "rowmap")}

    # ---- compact rows, forward
    want = np.full((Mp, lda), SENT_BITS, np.uint16)
    for k, m in means.items():
        want[T["rowmap"][k], :C] = m
    A = to_t(np.full((Mp, lda), SENT_BITS, np.uint16), dev)
    ok(L.mf_average_voxelization_rows_bf16_fwd(p(vd), ldv, p(pd), p(bd), n, C, B, D, p(tab["counts"]), p(tab["head"]),
                                               p(tab["link"]), p(tab["rowmap"]), p(A), lda, st()), L)
    same(to_bits(A), want, f"{what} C{C} rows fwd")
    # ---- compact rows, backward: gradient rows random where a voxel has its row, NaN where nothing may read
    named = T["rowvox"] >= 0
    gbits = np.full((Mp, lda), NAN_BITS, np.uint16)
    gbits[named, :C] = rand_bits(rs, int(named.sum()), C)
    gwant = np.full((n, ldg), SENT_BITS, np.uint16)
    gwant[:, :C] = grad_rows_ref(gbits, T["rowmap"], T, C)
    assert not gwant[T["key"] < 0, :C].any()
    gv = to_t(np.full((n, ldg), SENT_BITS, np.uint16), dev)
    dA = to_t(gbits, dev)
    ok(L.mf_average_voxelization_rows_bf16_bwd(p(dA), lda, p(pd), p(bd), p(tab["counts"]), p(tab["rowmap"]), n, C, B, D,
                                               p(gv), ldg, st()), L)
    same(to_bits(gv), gwant, f"{what} C{C} rows bwd")

    # ---- the dense form: x [B, D^3, ldx], columns < C the mean (zero where empty), columns >= C untouched
    xwant = np.full((BV, ldx), SENT_BITS, np.uint16)
    xwant[:, :C] = 0
    for k, m in means.items():
        xwant[k, :C] = m
    x = to_t(np.full((BV, ldx), SENT_BITS, np.uint16), dev)
    counts = torch.full((BV,), 77, dtype=torch.int32, device=dev)
    head = torch.full((BV,), 77, dtype=torch.int32, device=dev)
    link = torch.full((n,), 77, dtype=torch.int32, device=dev)
    ok(L.mf_average_voxelization_cl_bf16_fwd(p(vd), ldv, p(pd), p(bd), n, C, B, D, p(x), ldx, p(counts), p(head), p(link),
                                             st()), L)
    same(counts.cpu().numpy(), T["counts"], f"{what} C{C} dense counts")
    same(to_bits(x), xwant, f"{what} C{C} dense fwd")
    gx = rand_bits(rs, BV, ldx)
    gx[:, C:] = NAN_BITS
    gwant[:, :C] = grad_rows_ref(gx, np.arange(BV), T, C)
    gv = to_t(np.full((n, ldg), SENT_BITS, np.uint16), dev)
    gxd = to_t(gx, dev)
    ok(L.mf_average_voxelization_cl_bf16_bwd(p(gxd), ldx, p(pd), p(bd), p(tab["counts"]), n, C, B, D, p(gv), ldg, st()), L)
    same(to_bits(gv), gwant, f"{what} C{C} dense bwd")


# ------------------------------------------------------------------------------------- case 5: pack / unpack / cols
def pack_maps(Cout):
    """-> index arrays [8 classes, 8 slots] of the taps kx, ky, kz."""
    cls, slot = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    return ((cls & 1) + 2 * (slot & 1), ((cls >> 1) & 1) + 2 * ((slot >> 1) & 1), ((cls >> 2) & 1) + 2 * ((slot >> 2) & 1))


def pack_ref(W, Cs, c_off):
    """-> Wp [8][8 Cout][Cs], Wq [8][Cs][8 Cout] (the same values of W [Cout][w_cin][4][4][4], any dtype)."""
    Cout = W.shape[0]
    kx, ky, kz = pack_maps(Cout)
    Wc = W[:, c_off:c_off + Cs]                                  # [co][c][kx][ky][kz]
    g = Wc[:, :, kx, ky, kz]                                     # [co][c][cls][slot]
    Wp = np.ascontiguousarray(g.transpose(2, 3, 0, 1)).reshape(8, 8 * Cout, Cs)
    Wq = np.ascontiguousarray(g.transpose(2, 1, 3, 0)).reshape(8, Cs, 8 * Cout)
    return Wp, Wq


def unpack_ref(dWp, Cout, Cs):
    """The inverse map on [8][8 Cout][Cs] -> [Cout][Cs][4][4][4]."""
    kx, ky, kz = pack_maps(Cout)
    out = np.zeros((Cout, Cs, 4, 4, 4), dWp.dtype)
    out[:, :, kx, ky, kz] = dWp.reshape(8, 8, Cout, Cs).transpose(2, 3, 0, 1)
    return out


def pack_case(L, dev, st, Cout, Cs, w_cin, c_off, seed=31, what="pack"):
    rs = np.random.RandomState(seed)
    W = rand_f32(rs, Cout, w_cin, 4, 4, 4)
    Wb = bf16_bits(W)
    assert (Wb.astype(np.uint32) << 16 != W.view(np.uint32)).mean() > 0.9      # (the rounding has work to do)
    Wp_ref, Wq_ref = pack_ref(Wb, Cs, c_off)
    Wd = torch.from_numpy(W).to(dev)
    for with_q in (True, False):
        Wp = to_t(np.full((8, 8 * Cout, Cs), SENT_BITS, np.uint16), dev)
        Wq = to_t(np.full((8, Cs, 8 * Cout), SENT_BITS, np.uint16), dev)
        ok(L.mf_sparse_conv3_bf16_pack(p(Wd), Cout, Cs, w_cin, c_off, p(Wp), p(Wq) if with_q else None, st()), L)
        same(to_bits(Wp), Wp_ref, f"{what} Wp (Wq {with_q})")
        same(to_bits(Wq), Wq_ref if with_q else np.full_like(Wq_ref, SENT_BITS), f"{what} Wq (Wq {with_q})")
    # pack_cols: W2[tap * Cin + c][co]
    W2 = to_t(np.full((64 * Cs, Cout), SENT_BITS, np.uint16), dev)
    ok(L.mf_conv3d_k4s2_bf16_pack_cols(p(Wd), Cout, Cs, w_cin, c_off, p(W2), st()), L)
    W2_ref = Wb[:, c_off:c_off + Cs].reshape(Cout, Cs, 64).transpose(2, 1, 0).reshape(64 * Cs, Cout)
    same(to_bits(W2), W2_ref, f"{what} pack_cols")
    # unpack_dw: fp32, exact; the other channels of dW are not its to write
    dWp = rand_f32(rs, 8, 8 * Cout, Cs)
    dW = torch.full((Cout, w_cin, 4, 4, 4), SENT, device=dev)
    dWpd = torch.from_numpy(dWp).to(dev)
    ok(L.mf_sparse_conv3_bf16_unpack_dw(p(dWpd), Cout, Cs, w_cin, c_off, p(dW), st()), L)
    want = np.full((Cout, w_cin, 4, 4, 4), SENT, np.float32)
    want[:, c_off:c_off + Cs] = unpack_ref(dWp, Cout, Cs)
    same(dW.cpu().numpy().view(np.uint32), want.view(np.uint32), f"{what} unpack_dw")
    # round trip on values exact in bf16
    Wx = bf16_f32(rand_bits(rs, Cout, w_cin, 4, 4, 4))
    Wxd = torch.from_numpy(Wx).to(dev)
    Wp = torch.empty((8, 8 * Cout, Cs), dtype=BF, device=dev)
    ok(L.mf_sparse_conv3_bf16_pack(p(Wxd), Cout, Cs, w_cin, c_off, p(Wp), None, st()), L)
    back = torch.full((Cout, w_cin, 4, 4, 4), SENT, device=dev)
    Wp32 = Wp.float().contiguous()
    ok(L.mf_sparse_conv3_bf16_unpack_dw(p(Wp32), Cout, Cs, w_cin, c_off, p(back), st()), L)
    same(back.cpu().numpy()[:, c_off:c_off + Cs].view(np.uint32), Wx[:, c_off:c_off + Cs].view(np.uint32),
         f"{what} unpack(pack(W))")


def pack_refusal_case(L, dev, st):
    """Cs % 8 and c_off + Cs > w_cin: the error code, nothing written."""
    W = torch.zeros(8, 24, 4, 4, 4, device=dev)
    Wp = torch.full((8 * 64 * 24,), SENT, dtype=BF, device=dev)
    dW = torch.full((8, 24, 4, 4, 4), SENT, device=dev)
    dWp = torch.zeros(8 * 64 * 24, device=dev)
    assert L.mf_sparse_conv3_bf16_pack(p(W), 8, 12, 24, 0, p(Wp), None, st()) != 0            # Cs % 8
    assert L.mf_sparse_conv3_bf16_pack(p(W), 8, 16, 24, 16, p(Wp), None, st()) != 0           # c_off + Cs > w_cin
    assert L.mf_sparse_conv3_bf16_unpack_dw(p(dWp), 8, 16, 24, 16, p(dW), st()) != 0
    assert L.mf_conv3d_k4s2_bf16_pack_cols(p(W), 8, 16, 24, 16, p(Wp), st()) != 0
    assert float((Wp.float().cpu() - SENT).abs().max()) == 0.0 and float((dW.cpu() - SENT).abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------- case 6: reduce
def out_coords(Do):
    o = np.arange(Do ** 3)
    return o // (Do * Do), (o // Do) % Do, o % Do


def reduce_ref(Cbits, dense, bias, T, Cout, relu):
    """out[b][o][co] = bf16(relu?((sum over the taps t = (kx 4 + ky) 4 + kz in increasing t whose input voxel
    (2 o - 1 + k) lies inside the grid and has a row, of float32(C[row][slot(t) Cout + co])) + dense) + bias)."""
    B, D = T["B"], T["D"]
    Do, V = D // 2, D ** 3
    ox, oy, oz = out_coords(Do)
    s = np.zeros((B, Do ** 3, Cout), np.float32)
    rowmap = T["rowmap"].reshape(B, V)
    for t in range(64):
        kx, ky, kz = t >> 4, (t >> 2) & 3, t & 3
        slot = (kx >> 1) | ((ky >> 1) << 1) | ((kz >> 1) << 2)
        vx, vy, vz = 2 * ox - 1 + kx, 2 * oy - 1 + ky, 2 * oz - 1 + kz
        inside = (vx >= 0) & (vx < D) & (vy >= 0) & (vy < D) & (vz >= 0) & (vz < D)
        v = np.where(inside, (vx * D + vy) * D + vz, 0)
        rows = np.where(inside[None, :], rowmap[:, v], -1)           # [B, Vo]
        hit = rows >= 0
        s[hit] = s[hit] + bf16_f32(Cbits[rows[hit], slot * Cout:(slot + 1) * Cout])
    v = s + (dense if dense is not None else np.float32(0.0))
    v = v + (bias if bias is not None else np.float32(0.0))
    if relu:
        v = np.where(v > 0, v, np.float32(0.0)).astype(np.float32)
    return bf16_bits(v)


def c_rows(rs, T, width):
    """Random bf16 rows where a voxel has its row; NaN in every pad row and at or past class_off[8]."""
    named = T["rowvox"] >= 0
    bits = np.full((T["Mp"], width), NAN_BITS, np.uint16)
    bits[named] = rand_bits(rs, int(named.sum()), width, **WIDE)
    return bits


def reduce_case(L, dev, st, pts, bi, B, D, Cout, seed=41, what="reduce"):
    """mf_sparse_conv3_bf16_reduce on the reference's row map: dense / bias present or NULL x ReLU on / off."""
    rs = np.random.RandomState(seed)
    n, Vo = len(pts), (D // 2) ** 3
    T = tables_ref(pts, bi, B, D)
    ws = Workspace(L, dev, n, B, D).put(T)
    Cbits = c_rows(rs, T, 8 * Cout)
    dense, bias = rand_f32(rs, B, Vo, Cout), rand_f32(rs, Cout)
    Cd, dd, bd = to_t(Cbits, dev), torch.from_numpy(dense).to(dev), torch.from_numpy(bias).to(dev)
    for use_dense in (True, False):
        for use_bias in (True, False):
            for relu in (1, 0):
                out = to_t(np.full((B, Vo, Cout), SENT_BITS, np.uint16), dev)
                ok(L.mf_sparse_conv3_bf16_reduce(p(Cd), p(dd) if use_dense else None, p(bd) if use_bias else None, ws.ptr(),
                                                 n, B, D, Cout, relu, p(out), st()), L)
                got = to_bits(out)
                tag = f"{what} B{B} D{D} Cout{Cout} dense={use_dense} bias={use_bias} relu={relu}"
                assert not np.isnan(bf16_f32(got)).any(), f"{tag}: NaN (a pad row was read)"
                same(got, reduce_ref(Cbits, dense if use_dense else None, bias if use_bias else None, T, Cout, relu), tag)


def reduce_refusal_case(L, dev, st):
    """Cout = 264 (not a multiple of 256): the error code, out untouched."""
    pts, bi = points_faces(1, 6)
    ws = Workspace(L, dev, len(pts), 1, 6).put(tables_ref(pts, bi, 1, 6))
    Cd = torch.zeros((max_rows(len(pts)), 8 * 264), dtype=BF, device=dev)
    out = torch.full((1, 27, 264), SENT, dtype=BF, device=dev)
    assert L.mf_sparse_conv3_bf16_reduce(p(Cd), None, None, ws.ptr(), len(pts), 1, 6, 264, 1, p(out), st()) != 0
    assert float((out.float().cpu() - SENT).abs().max()) == 0.0


# ----------------------------------------------------------------------------------------------- case 7: gather_dy
def gather_ref(dzbits, T, Cout):
    """dYg[row][slot Cout + co] = dz[b][o][co], o = ((v + 1) >> 1) - (slot bit) per axis; zero where o lies outside
    the output grid and in pad rows.  -> rows [0, class_off[8])."""
    B, D = T["B"], T["D"]
    Do, V = D // 2, D ** 3
    R = int(T["class_off"][8])
    out = np.zeros((R, 8, Cout), np.uint16)
    bv = T["rowvox"][:R]
    rows = np.flatnonzero(bv >= 0)
    b, v = bv[rows] // V, bv[rows] % V
    vx, vy, vz = v // (D * D), (v // D) % D, v % D
    dz = dzbits.reshape(B, Do ** 3, Cout)
    for slot in range(8):
        ox, oy, oz = ((vx + 1) >> 1) - (slot & 1), ((vy + 1) >> 1) - ((slot >> 1) & 1), ((vz + 1) >> 1) - ((slot >> 2) & 1)
        inside = (ox >= 0) & (ox < Do) & (oy >= 0) & (oy < Do) & (oz >= 0) & (oz < Do)
        out[rows[inside], slot] = dz[b[inside], ((ox * Do + oy) * Do + oz)[inside]]
    return out.reshape(R, 8 * Cout)


def gather_case(L, dev, st, pts, bi, B, D, Cout, seed=51, what="gather_dy"):
    rs = np.random.RandomState(seed)
    n, Vo = len(pts), (D // 2) ** 3
    T = tables_ref(pts, bi, B, D)
    ws = Workspace(L, dev, n, B, D).put(T)
    dz = rand_bits(rs, B, Vo, Cout, zeros=0.0)            # (no zeros: a missing value cannot pass for a pad's)
    dzd = to_t(dz, dev)
    dYg = to_t(np.full((T["Mp"], 8 * Cout), SENT_BITS, np.uint16), dev)
    ok(L.mf_sparse_conv3_bf16_gather_dy(p(dzd), ws.ptr(), n, B, D, Cout, p(dYg), st()), L)
    R = int(T["class_off"][8])
    assert R > int((T["rowvox"] >= 0).sum()), "the case has pad rows"
    same(to_bits(dYg)[:R], gather_ref(dz, T, Cout), f"{what} B{B} D{D} Cout{Cout}")


# -------------------------------------------------------------------------------------------------- case 8: col2im
def col2im_ref(Tbits, B, D, Cin):
    """dx[b][v][c] = bf16 of the fp32 sum in slot order 0..7 of T[b][o(v, slot)][tap(v, slot) Cin + c]; slots whose
    output voxel lies outside are skipped."""
    Do, V = D // 2, D ** 3
    Tf = bf16_f32(Tbits).reshape(B, Do ** 3, 64, Cin)
    v = np.arange(V)
    vx, vy, vz = v // (D * D), (v // D) % D, v % D
    px, py, pz = (vx + 1) & 1, (vy + 1) & 1, (vz + 1) & 1
    acc = np.zeros((B, V, Cin), np.float32)
    for slot in range(8):
        ax, ay, az = slot & 1, (slot >> 1) & 1, (slot >> 2) & 1
        ox, oy, oz = ((vx + 1) >> 1) - ax, ((vy + 1) >> 1) - ay, ((vz + 1) >> 1) - az
        inside = (ox >= 0) & (ox < Do) & (oy >= 0) & (oy < Do) & (oz >= 0) & (oz < Do)
        tap = ((px + 2 * ax) * 4 + (py + 2 * ay)) * 4 + (pz + 2 * az)
        o = (ox * Do + oy) * Do + oz
        acc[:, inside] = acc[:, inside] + Tf[:, o[inside], tap[inside]]
    return bf16_bits(acc)


def col2im_case(L, dev, st, B, D, Cin, seed=61, what="col2im"):
    rs = np.random.RandomState(seed)
    Vo = (D // 2) ** 3
    Tb = rand_bits(rs, B * Vo, 64 * Cin, **WIDE)
    Td = to_t(Tb, dev)
    dx = to_t(np.full((B, D ** 3, Cin), SENT_BITS, np.uint16), dev)
    ok(L.mf_conv3d_k4s2_bf16_col2im(p(Td), B, D, Cin, p(dx), st()), L)
    same(to_bits(dx), col2im_ref(Tb, B, D, Cin), f"{what} B{B} D{D} Cin{Cin}")


def col2im_refusal_case(L, dev, st):
    Td = torch.zeros((2 * 27, 64 * 12), dtype=BF, device=dev)
    dx = torch.full((2, 216, 12), SENT, dtype=BF, device=dev)
    assert L.mf_conv3d_k4s2_bf16_col2im(p(Td), 2, 6, 12, p(dx), st()) != 0     # Cin = 12
    assert float((dx.float().cpu() - SENT).abs().max()) == 0.0


# -------------------------------------------------------------------------------------------- case 9: the wiring
def _fold(S, extra, K):
    """S' with 2 K 2^-24 S' = 2 K 2^-24 S + extra: a further absolute term carried through BB.assert_within."""
    return S + extra / (2.0 * K * BB.U32)


def wiring_case(K, dev, seed=71, what="SparseConv3"):
    """bf16_ops.SparseConv3 end to end, EVERY element: with the stages pinned bit for bit this checks that the operator
    hands the right table to the right engine (Wp / Wq, t_group / t_range, c_off of the occupancy channels).

    Reference: float64 dense convolution (bf16_bound.conv_ref) over the grid of the REFERENCE's bf16 mean rows plus
    h_occ, on the bf16-rounded weight.  S = the same contraction on absolute values, S_sp its part over the Cs
    voxelized channels; u = 2^-8 (bf16), 2^-24 the fp32 accumulator's unit (bf16_bound's 2 K 2^-24 S for K terms):

      out    |got - ref| <= u |ref| + u (1 + u) S_sp + 2 K 2^-24 S, K = 64 (Cs + Co) + 1: one final rounding; every row
             of C was rounded to bf16 before the taps were summed (u on its own value, itself within (1 + u) of S_sp's
             share); the fp32 sums of all 64 (Cs + Co) products and the bias
      mask   may differ from the reference's only where the reference is within that bound of zero
      dW[:, :Cs]  with the OPERATOR's mask: fp32 sums over the class's padded rows, 2 K 2^-24 S, K = that row count
      dW[:, Cs:]  the dense engine's weight gradient: K = B Do^3 + split (bf16_cases.conv_case)
      dfeat  u |ref| + u (1 + u) S / count + 2 K 2^-24 S / count, K = 8 Cout: dA is rounded to bf16, then the
             quotient by the count is
      docc   the same form without the count: T is rounded to bf16, then the sum of its 8 slots is; K = Cout."""
    B, D, Cs, Co, Cout = 2, 8, 16, 8, 256
    Do, V = D // 2, D ** 3
    rs = np.random.RandomState(seed)
    pts, bi = points_faces(B, D)
    n = len(pts)
    T = tables_ref(pts, bi, B, D)
    fbits, hbits = rand_bits(rs, n, Cs), rand_bits(rs, B, V, Co)
    W = (rs.standard_normal((Cout, Cs + Co, 4, 4, 4)) * (64 * (Cs + Co)) ** -0.5).astype(np.float32)
    bias = (rs.standard_normal(Cout) * 0.1).astype(np.float32)
    gbits = rand_bits(rs, B, Do ** 3, Cout)

    feat = to_t(fbits, dev).requires_grad_(True)
    hocc = to_t(hbits, dev).requires_grad_(True)
    Wt = torch.from_numpy(W).to(dev).requires_grad_(True)
    bt = torch.from_numpy(bias).to(dev).requires_grad_(True)
    out = K.SparseConv3.apply(feat, hocc, torch.from_numpy(pts).to(dev), torch.from_numpy(bi).to(dev), Wt, bt, B, D)
    assert out.shape == (B, Do ** 3, Cout) and out.dtype == BF
    out.backward(to_t(gbits, dev))

    # ---- the reference grid: the reference's own mean rows (bit-exact stage 4) | h_occ
    x = np.zeros((B * V, Cs + Co), np.float32)
    for k, m in mean_rows_ref(fbits, T, Cs).items():
        x[k, :Cs] = bf16_f32(m)
    x[:, Cs:] = bf16_f32(hbits).reshape(B * V, Co)
    x = torch.from_numpy(x).reshape(B, V, Cs + Co)
    x_sp = x.clone()
    x_sp[:, :, Cs:] = 0
    Wb = torch.from_numpy(bf16_f32(bf16_bits(W)))
    r0 = BB.conv_ref(x, Wb, torch.from_numpy(bias), D, GEOM)
    S_sp = BB.conv_ref(x_sp, Wb, None, D, GEOM)["Sy"]
    Kf = 64 * (Cs + Co) + 1
    S_out = _fold(r0["Sy"], BB.U16 * (1 + BB.U16) * S_sp, Kf)
    BB.assert_within(out, F.relu(r0["y"]), S_out, Kf, f"{what} out")
    mask = BB.relu_mask_agrees(out, r0["y"], S_out, Kf, f"{what}")

    # ---- gradients, with the operator's own mask
    dz = torch.from_numpy(bf16_f32(gbits)).double() * mask
    r = BB.conv_ref(x, Wb, None, D, GEOM, dz_cl=dz)
    dW = Wt.grad.detach().cpu()
    assert dW.shape == W.shape and dW.dtype == torch.float32
    co = T["class_off"]
    for c in range(8):
        sl = (slice(None), slice(0, Cs), slice(c & 1, 4, 2), slice((c >> 1) & 1, 4, 2), slice((c >> 2) & 1, 4, 2))
        BB.assert_within(dW[sl], r["dw"][sl], r["Sdw"][sl], max(int(co[c + 1] - co[c]), 1), f"{what} dW voxelized, class {c}")
    split = int(K._lib.lib().mf_conv3d_bf16_wgrad_default_split(B, Co, Cout, Do, 4))
    BB.assert_within(dW[:, Cs:], r["dw"][:, Cs:], r["Sdw"][:, Cs:], B * Do ** 3 + split, f"{what} dW occupancy (split {split})")
    # dfeat: the voxel's gradient row / count
    key = T["key"]
    inside = torch.from_numpy(key >= 0)
    kk = torch.from_numpy(np.where(key >= 0, key, 0))
    cnt = torch.from_numpy(np.maximum(T["counts"][np.where(key >= 0, key, 0)], 1)).double()[:, None]
    ref = r["dx"].reshape(B * V, -1)[kk, :Cs] / cnt * inside[:, None]
    S = r["Sdx"].reshape(B * V, -1)[kk, :Cs] / cnt * inside[:, None]
    Kd = 8 * Cout
    BB.assert_within(feat.grad, ref, _fold(S, BB.U16 * (1 + BB.U16) * S, Kd), Kd, f"{what} dfeat")
    assert float(feat.grad[~inside.to(feat.grad.device)].float().abs().max()) == 0.0
    # docc
    ref, S = r["dx"][:, :, Cs:], r["Sdx"][:, :, Cs:]
    BB.assert_within(hocc.grad, ref, _fold(S, BB.U16 * (1 + BB.U16) * S, Cout), Cout, f"{what} docc")
    return {k: v for k, v in BB.RATIOS.items() if k.startswith(what)}

"""TEST INFRASTRUCTURE: the rules of the ICC launch plan (csrc/icc.hip: icc_plan, read_icc_knobs) restated in Python,
and the library's own answer (mf_icc_plan: host arithmetic over a descriptor, no launch, null pointers allowed).
tests/test_emul_icc_plan.py holds one against the other on the CPU; the MI355X tests assert single slots of the
library that ran."""
import ctypes
import math

import numpy as np

from morefusion_amd import _lib

SLOTS = ("single_pass", "launches", "variant", "ws_bytes", "n_tab", "nbins", "hmax", "lds_fused", "lds_tile", "lds_accum",
         "NB", "xcd_order", "bin_cap_force", "uniform_ns", "rec_n")
TILE_ACCUM, FUSED, FUSED_BIG = 0, 1, 2      # slot "variant": the kernel(s) behind k_icc_bin


def desc(n_objects, n_scenes, max_ns, n_points=1000, dim=32, thr=2.0, ne_binary=1, flags=0):
    """A descriptor that is all numbers: every array pointer NULL (a plan reads none of them)."""
    d = _lib.IccBatch(None, None, None, None, None, None, None, None, n_objects, n_scenes, n_points, dim, max_ns,
                      float(thr), 0.02, ne_binary)
    d.flags = flags
    return d


def query(L, d, n=len(SLOTS)):
    """mf_icc_plan's answer -> dict of the first n slots, or None where the library refuses the descriptor."""
    out = (ctypes.c_int64 * len(SLOTS))(*([-7] * len(SLOTS)))
    rc = L.mf_icc_plan(ctypes.byref(d), out, n)
    if rc < 0:
        return None
    assert rc == len(SLOTS) and all(v == -7 for v in out[n:])
    return dict(zip(SLOTS[:n], out[:n]))


def ksize_host(thr):
    """Upper bound of a grid's TDF kernel size: ceil(thr * 1.000001) in float32, made odd."""
    ks = int(math.ceil(np.float32(thr) * np.float32(1.000001)))
    return ks + 1 if ks % 2 == 0 else ks


def align256(x):
    return (x + 255) & ~255


def plan(d, general=None, bin_cap=None, dbg=0, lds_pad=0):
    """The plan restated.  ``general`` / ``bin_cap``: the MF_ICC_GENERAL / MF_ICC_BIN_CAP strings (None = not set; a
    number other than 0 asks for the two-kernel path, forces every bin's capacity); ``dbg`` / ``lds_pad``: MF_ICC_DEBUG /
    MF_ICC_LDS_PAD as a build with -DMF_ICC_DEBUG_BUILD=1 reads them (every other build: 0)."""
    O, S, P, D, N, thr = d.n_objects, d.n_scenes, d.n_points, d.dim, d.max_scene_objects, d.voxel_threshold
    force = int(bin_cap) if bin_cap else 0
    # single pass: {0,1} no-entry grids, one voxel of a half-plane per lane of 512, and nobody asked for the other path
    single = bool(d.grid_ne_binary) and -(-D // 2) * D <= 512 and not (general and int(general) != 0)
    ks = ksize_host(thr) if thr > 0 else 0
    if not (O > 0 and S > 0 and 0 < D <= 64 and P >= 0 and 0 < N <= (128 if single else 64) and thr > 0 and ks <= 7
            and P * 343 < 4294967295 and P < 1 << 27 and d.flags == 0):
        return None
    hmax = ks // 2
    nbins = 2 * (D + 2 * hmax) + 1                                    # two y-halves per x-plane + the overflow counter
    n_tab = (-(-(N * P) // 1024) + O * N + O + 7) & ~7                # chunks of 1024 points, a multiple of 8
    V = D ** 3
    rows2 = min(N, 64) * 32 * 13 * 4                                  # collision rows: 1664 B per object, 64 at a time
    tile_words = (-(-D // 2) + 4) * (D + 4)                           # padded half-plane of the fused kernel
    sumP = N * P
    rec_n = (nbins - 1) * ((0 if force > 0 else sumP // 8) + 2 * O * ((force if force > 0 else 64) + 1)) + 2 * sumP
    arrays = [2 * O * V * 8, 2 * 2 * O * 4, 2 * O * 12 * 4, O * 16, S * 4, 2 * O * 66 * 8, 2 * O * N * 12 * 8, O * 21 * 4,
              O * 16, n_tab * 16, n_tab * 16, 2 * 2 * O * nbins * 4, 2 * O * 4, 2 * O * 4, 2 * O * 8, rec_n * 16]
    return dict(
        single_pass=int(single), launches=2 if single else 3,
        variant=TILE_ACCUM if not single else FUSED_BIG if N > 64 else FUSED,
        ws_bytes=sum(align256(a) for a in arrays), n_tab=n_tab, nbins=nbins, hmax=hmax,
        lds_fused=4 * tile_words * 4 + rows2 + lds_pad if single else 0,
        lds_tile=-(-D // 2) * D * 2 * 4, lds_accum=rows2, NB=-(-V // 1024),
        xcd_order=int((O >= 32 or bool(dbg & 2048)) and not dbg & 4096),
        bin_cap_force=force, uniform_ns=N if S * N == O else 0, rec_n=rec_n)

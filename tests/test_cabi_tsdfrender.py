"""The TSDF-render entry points of the C ABI without a GPU: the summary's size is host-only arithmetic, every bad argument
is refused on the host, before any launch, with the library's invalid-argument code and the function's name in the error
string; null arrays with valid scalars are refused too, not dereferenced."""
import pytest

import morefusion_amd as mf

INVALID = -1  # -(int)hipErrorInvalidValue
P = 0x1000    # a non-null pointer that must never be dereferenced: every call below is refused first
NAN = float("nan")

VOLUME = dict(nx=8, ny=8, nz=8)
SUMMARY = dict(volume=P, **VOLUME, B=8, summary=P, stream=None)
RENDER = dict(volume=P, **VOLUME, ox=0.0, oy=0.0, oz=0.0, pitch=0.1, step=0.05, min_depth=0.0, max_depth=10.0,
              max_steps=64, H=24, W=32, fx=30.0, fy=30.0, cx=16.0, cy=12.0, T=P, summary=P, B=8, labels=None,
              min_count=1, depth_out=P, code_out=None, label_out=None, stats_out=None, stream=None)

BAD_DIMS = [dict(nx=1), dict(ny=1), dict(nz=0), dict(nx=-8), dict(nx=2048, ny=1024, nz=1024)]
BAD_B = [dict(B=0), dict(B=1), dict(B=3), dict(B=6), dict(B=32), dict(B=-8)]


def _call(name, base, **change):
    L = mf._lib.lib()
    rc = getattr(L, name)(*dict(base, **change).values())
    return rc, L.mf_last_error_string()


def test_summary_bytes():
    size = mf._lib.lib().mf_tsdf_summary_bytes
    assert size(37, 29, 33, 8) == 5 * 4 * 4 and size(37, 29, 33, 4) == 9 * 7 * 8 and size(37, 29, 33, 2) == 18 * 14 * 16
    assert size(2, 2, 2, 16) == 1 and size(17, 18, 19, 16) == 1 * 2 * 2 and size(256, 256, 256, 8) == 32 ** 3
    assert size(2047, 1024, 1024, 2) == 1023 * 512 * 512
    for change in BAD_DIMS + BAD_B:
        assert size(*dict(dict(VOLUME, B=8), **change).values()) < 0, change


@pytest.mark.parametrize("change", BAD_DIMS + BAD_B + [dict(volume=None), dict(summary=None)], ids=str)
def test_block_summary_refuses(change):
    rc, msg = _call("mf_tsdf_block_summary", SUMMARY, **change)
    assert rc == INVALID and b"mf_tsdf_block_summary" in msg


@pytest.mark.parametrize("change", BAD_DIMS + BAD_B + [
    dict(pitch=0.0), dict(pitch=NAN), dict(step=0.0), dict(step=NAN), dict(min_depth=-0.1), dict(min_depth=10.0),
    dict(max_depth=NAN), dict(max_steps=0), dict(max_steps=65537), dict(H=0), dict(W=4097), dict(fx=0.0), dict(fy=NAN),
    dict(volume=None), dict(T=None), dict(summary=None), dict(depth_out=None), dict(labels=P), dict(label_out=P),
    dict(labels=P, label_out=P, min_count=0), dict(labels=P, label_out=P, min_count=-2)], ids=str)
def test_render_refuses(change):
    rc, msg = _call("mf_tsdf_render", RENDER, **change)
    assert rc == INVALID and b"mf_tsdf_render" in msg


def test_the_largest_allowed_scalars_reach_the_null_array_check():
    """2^31 - 2^20 voxels, B = 16, the step cap at its limit, min_count unused without labels: accepted as scalars -- the
    refusal names the null arrays."""
    big = dict(nx=2047, ny=1024, nz=1024)
    rc, msg = _call("mf_tsdf_block_summary", SUMMARY, **big, B=16, summary=None)
    assert rc == INVALID and b"null" in msg
    rc, msg = _call("mf_tsdf_render", RENDER, **big, B=16, H=4096, W=4096, max_steps=65536, max_depth=float("inf"),
                    min_count=0, depth_out=None)
    assert rc == INVALID and b"null" in msg

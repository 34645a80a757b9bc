"""The TSDF-colour entry points of the C ABI without a GPU: every bad argument is refused on the host, before any
launch, with the library's invalid-argument code and the function's name in the error string; null and misaligned
arrays with valid scalars are refused too, not dereferenced."""
import pytest

import morefusion_amd as mf

INVALID = -1  # -(int)hipErrorInvalidValue
P = 0x1000    # a non-null, aligned pointer that must never be dereferenced: every call below is refused first
NAN = float("nan")

VOLUME = dict(nx=8, ny=8, nz=8)
GEOMETRY = dict(ox=0.0, oy=0.0, oz=0.0, pitch=0.1)
CAMERA = dict(H=24, W=32, fx=30.0, fy=30.0, cx=16.0, cy=12.0, T=P)
# the argument lists, in the header's order
INTEGRATE = dict(colors=P, **VOLUME, **GEOMETRY, truncation=0.4, max_weight=64.0, depth=P, rgb=P, **CAMERA,
                 skip_flag=None, stream=None)
COLOR_IMAGE = dict(colors=P, **VOLUME, **GEOMETRY, depth=P, **CAMERA, out=P, stream=None)
SAMPLE = dict(colors=P, **VOLUME, **GEOMETRY, points=P, N=100, out=P, stream=None)

BAD_DIMS = [dict(nx=1), dict(ny=1), dict(nz=0), dict(nx=-8), dict(nx=2048, ny=1024, nz=1024)]
BAD_PITCH = [dict(pitch=0.0), dict(pitch=-0.1), dict(pitch=NAN)]
BAD_CAMERA = [dict(H=0), dict(W=0), dict(H=4097), dict(fx=0.0), dict(fy=-1.0), dict(fx=NAN)]
MISALIGNED = [dict(colors=P + 4), dict(colors=P + 8)]


def _call(name, base, **change):
    L = mf._lib.lib()
    rc = getattr(L, name)(*dict(base, **change).values())
    return rc, L.mf_last_error_string()


def _nulls(base, optional=()):
    return [{k: None} for k, v in base.items() if v == P and k not in optional]


@pytest.mark.parametrize("change", BAD_DIMS + BAD_PITCH + BAD_CAMERA + MISALIGNED + [
    dict(truncation=0.0), dict(truncation=NAN), dict(max_weight=0.5), dict(max_weight=NAN)] + _nulls(INTEGRATE), ids=str)
def test_integrate_colors_refuses(change):
    rc, msg = _call("mf_tsdf_integrate_colors", INTEGRATE, **change)
    assert rc == INVALID and b"mf_tsdf_integrate_colors" in msg


@pytest.mark.parametrize("change", BAD_DIMS + BAD_PITCH + BAD_CAMERA + MISALIGNED + [dict(out=P + 2)]
                         + _nulls(COLOR_IMAGE), ids=str)
def test_color_image_refuses(change):
    rc, msg = _call("mf_tsdf_color_image", COLOR_IMAGE, **change)
    assert rc == INVALID and b"mf_tsdf_color_image" in msg


@pytest.mark.parametrize("change", BAD_DIMS + BAD_PITCH + MISALIGNED + [
    dict(N=0), dict(N=-1), dict(N=2 ** 31), dict(N=2 ** 40), dict(out=P + 1)] + _nulls(SAMPLE), ids=str)
def test_sample_colors_refuses(change):
    rc, msg = _call("mf_tsdf_sample_colors", SAMPLE, **change)
    assert rc == INVALID and b"mf_tsdf_sample_colors" in msg


def test_every_array_argument_is_covered():
    assert len(_nulls(INTEGRATE)) == 4 and len(_nulls(COLOR_IMAGE)) == 4 and len(_nulls(SAMPLE)) == 3


def test_the_largest_allowed_scalars_reach_the_null_array_check():
    """2^31 - 2^20 voxels, 4096 x 4096 images, N = 2^31 - 1: accepted as scalars -- the refusal names the null arrays;
    and with every array given, the misaligned one."""
    big = dict(nx=2047, ny=1024, nz=1024)
    rc, msg = _call("mf_tsdf_integrate_colors", INTEGRATE, **big, H=4096, W=4096, colors=None)
    assert rc == INVALID and b"null" in msg
    rc, msg = _call("mf_tsdf_color_image", COLOR_IMAGE, **big, H=4096, W=4096, out=None)
    assert rc == INVALID and b"null" in msg
    rc, msg = _call("mf_tsdf_sample_colors", SAMPLE, **big, N=2 ** 31 - 1, out=None)
    assert rc == INVALID and b"null" in msg
    rc, msg = _call("mf_tsdf_sample_colors", SAMPLE, **big, N=2 ** 31 - 1, colors=P + 8)
    assert rc == INVALID and b"aligned" in msg

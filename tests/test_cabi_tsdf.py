"""The TSDF entry points of the C ABI without a GPU: every bad argument is refused on the host, before any launch, with
the library's invalid-argument code and the function's name in the error string; null arrays with valid scalars are
refused too, not dereferenced."""
import pytest

import morefusion_amd as mf

INVALID = -1  # -(int)hipErrorInvalidValue
P = 0x1000    # a non-null pointer that must never be dereferenced: every call below is refused first

# mf_tsdf_integrate(volume, nx, ny, nz, ox, oy, oz, pitch, truncation, max_weight, depth, H, W, fx, fy, cx, cy, T,
#                   skip_flag, stream)
INTEGRATE = dict(volume=P, nx=8, ny=8, nz=8, ox=0.0, oy=0.0, oz=0.0, pitch=0.1, truncation=0.4, max_weight=64.0,
                 depth=P, H=24, W=32, fx=30.0, fy=30.0, cx=16.0, cy=12.0, T=P, skip_flag=None, stream=None)
# mf_tsdf_raycast(volume, nx, ny, nz, ox, oy, oz, pitch, step, min_depth, max_depth, max_steps, H, W, fx, fy, cx, cy,
#                 T, depth_out, code_out, stream)
RAYCAST = dict(volume=P, nx=8, ny=8, nz=8, ox=0.0, oy=0.0, oz=0.0, pitch=0.1, step=0.2, min_depth=0.0, max_depth=10.0,
               max_steps=16, H=24, W=32, fx=30.0, fy=30.0, cx=16.0, cy=12.0, T=P, depth_out=P, code_out=None,
               stream=None)
NAN = float("nan")
BAD_VOLUME = [dict(nx=1), dict(ny=1), dict(nz=0), dict(nx=2048, ny=1024, nz=1024), dict(pitch=0.0), dict(pitch=-0.1),
              dict(pitch=NAN)]
BAD_CAMERA = [dict(H=0), dict(W=0), dict(H=4097), dict(fx=0.0), dict(fy=-1.0), dict(fx=NAN)]


def _call(name, base, **change):
    L = mf._lib.lib()
    rc = getattr(L, name)(*dict(base, **change).values())
    return rc, L.mf_last_error_string()


@pytest.mark.parametrize("change", BAD_VOLUME + BAD_CAMERA + [
    dict(truncation=0.0), dict(truncation=NAN), dict(max_weight=0.5), dict(max_weight=NAN),
    dict(volume=None), dict(depth=None), dict(T=None)], ids=str)
def test_integrate_refuses(change):
    rc, msg = _call("mf_tsdf_integrate", INTEGRATE, **change)
    assert rc == INVALID and b"mf_tsdf_integrate" in msg


@pytest.mark.parametrize("change", BAD_VOLUME + BAD_CAMERA + [
    dict(step=0.0), dict(step=NAN), dict(min_depth=-0.1), dict(min_depth=10.0), dict(max_depth=NAN),
    dict(max_steps=0), dict(max_steps=65537), dict(volume=None), dict(T=None), dict(depth_out=None)], ids=str)
def test_raycast_refuses(change):
    rc, msg = _call("mf_tsdf_raycast", RAYCAST, **change)
    assert rc == INVALID and b"mf_tsdf_raycast" in msg


def test_the_largest_allowed_scalars_reach_the_null_array_check():
    """2^31 - 2^20 voxels, max_steps = 65536, an unbounded max_depth: accepted as scalars -- the refusal names the
    null arrays."""
    rc, msg = _call("mf_tsdf_integrate", INTEGRATE, nx=2047, ny=1024, nz=1024, volume=None, depth=None, T=None)
    assert rc == INVALID and b"null" in msg
    rc, msg = _call("mf_tsdf_raycast", RAYCAST, nx=2047, ny=1024, nz=1024, max_steps=65536, max_depth=float("inf"),
                    H=4096, W=4096, volume=None, T=None, depth_out=None)
    assert rc == INVALID and b"null" in msg

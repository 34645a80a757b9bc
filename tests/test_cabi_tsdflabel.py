"""The TSDF-label entry points of the C ABI without a GPU: every bad argument is refused on the host, before any
launch, with the library's invalid-argument code and the function's name in the error string; null arrays with valid
scalars are refused too, not dereferenced."""
import pytest

import morefusion_amd as mf

INVALID = -1  # -(int)hipErrorInvalidValue
P = 0x1000    # a non-null pointer that must never be dereferenced: every call below is refused first
NAN = float("nan")

VOLUME = dict(nx=8, ny=8, nz=8)
GEOMETRY = dict(ox=0.0, oy=0.0, oz=0.0, pitch=0.1)
CAMERA = dict(H=24, W=32, fx=30.0, fy=30.0, cx=16.0, cy=12.0, T=P)
# the argument lists, in the header's order
INTEGRATE = dict(volume=P, labels=P, **VOLUME, **GEOMETRY, truncation=0.4, max_weight=64.0, depth=P, **CAMERA,
                 label_image=P, max_count=64, skip_flag=None, stream=None)
LABEL_IMAGE = dict(labels=P, **VOLUME, **GEOMETRY, depth=P, **CAMERA, min_count=1, out=P, stream=None)
STATS = dict(volume=P, labels=P, **VOLUME, min_weight=1.0, min_count=1, ids=P, B=4, table=P, stream=None)
PUBLISH = dict(volume=P, labels=P, **VOLUME, **GEOMETRY, ids=P, grid_pitch=P, center_map=P, T_map_to_sensor=P,
               T_sensor_to_map=P, min_weight=1.0, min_count=1, empty_above=0.5, ground_z=0.0, flags=3, B=2, D=32,
               origin=P, grid_target=P, grid_noentry=P, grid_nontarget_empty=P, stream=None)

BAD_DIMS = [dict(nx=1), dict(ny=1), dict(nz=0), dict(nx=-8), dict(nx=2048, ny=1024, nz=1024)]
BAD_PITCH = [dict(pitch=0.0), dict(pitch=-0.1), dict(pitch=NAN)]
BAD_CAMERA = [dict(H=0), dict(W=0), dict(H=4097), dict(fx=0.0), dict(fy=-1.0), dict(fx=NAN)]


def _call(name, base, **change):
    L = mf._lib.lib()
    rc = getattr(L, name)(*dict(base, **change).values())
    return rc, L.mf_last_error_string()


def _nulls(base, optional=()):
    return [{k: None} for k, v in base.items() if v == P and k not in optional]


@pytest.mark.parametrize("change", BAD_DIMS + BAD_PITCH + BAD_CAMERA + [
    dict(truncation=0.0), dict(truncation=NAN), dict(max_weight=0.5), dict(max_weight=NAN), dict(max_count=0),
    dict(max_count=-3)] + _nulls(INTEGRATE), ids=str)
def test_integrate_labels_refuses(change):
    rc, msg = _call("mf_tsdf_integrate_labels", INTEGRATE, **change)
    assert rc == INVALID and b"mf_tsdf_integrate_labels" in msg


@pytest.mark.parametrize("change", BAD_DIMS + BAD_PITCH + BAD_CAMERA + [dict(min_count=0)] + _nulls(LABEL_IMAGE), ids=str)
def test_label_image_refuses(change):
    rc, msg = _call("mf_tsdf_label_image", LABEL_IMAGE, **change)
    assert rc == INVALID and b"mf_tsdf_label_image" in msg


@pytest.mark.parametrize("change", BAD_DIMS + [dict(B=0), dict(B=65), dict(B=-1), dict(min_weight=0.0),
                                               dict(min_weight=NAN), dict(min_count=0)] + _nulls(STATS), ids=str)
def test_instance_stats_refuses(change):
    rc, msg = _call("mf_tsdf_instance_stats", STATS, **change)
    assert rc == INVALID and b"mf_tsdf_instance_stats" in msg


@pytest.mark.parametrize("change", BAD_DIMS + BAD_PITCH + [
    dict(B=0), dict(B=65), dict(D=0), dict(D=-1), dict(D=257), dict(flags=4), dict(flags=-1), dict(min_weight=0.0),
    dict(min_weight=NAN), dict(min_count=0)] + _nulls(PUBLISH), ids=str)
def test_publish_grids_refuses(change):
    rc, msg = _call("mf_tsdf_publish_grids", PUBLISH, **change)
    assert rc == INVALID and b"mf_tsdf_publish_grids" in msg


def test_the_largest_allowed_scalars_reach_the_null_array_check():
    """2^31 - 2^20 voxels, B = 64, D = 256, a NaN ground_z and empty_above (they only fail comparisons): accepted as
    scalars -- the refusal names the null arrays."""
    big = dict(nx=2047, ny=1024, nz=1024)
    rc, msg = _call("mf_tsdf_integrate_labels", INTEGRATE, **big, H=4096, W=4096, max_count=2 ** 31 - 1, volume=None)
    assert rc == INVALID and b"null" in msg
    rc, msg = _call("mf_tsdf_label_image", LABEL_IMAGE, **big, H=4096, W=4096, min_count=2 ** 31 - 1, out=None)
    assert rc == INVALID and b"null" in msg
    rc, msg = _call("mf_tsdf_instance_stats", STATS, **big, B=64, table=None)
    assert rc == INVALID and b"null" in msg
    rc, msg = _call("mf_tsdf_publish_grids", PUBLISH, **big, B=64, D=256, ground_z=NAN, empty_above=NAN, origin=None)
    assert rc == INVALID and b"null" in msg

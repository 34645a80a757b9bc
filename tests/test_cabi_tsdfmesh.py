"""The TSDF-mesh entry points of the C ABI without a GPU: every bad scalar is refused on the host, before any launch,
with the library's invalid-argument code and the function's name in the error string; null or misaligned arrays with
valid scalars are refused too, not dereferenced."""
import pytest

import morefusion_amd as mf

INVALID = -1  # -(int)hipErrorInvalidValue
P = 0x1000    # a non-null, 16-byte aligned pointer that must never be dereferenced: every call below is refused first

# mf_tsdfmesh_count(volume, nx, ny, nz, min_weight, workspace, totals, stream)
COUNT = dict(volume=P, nx=8, ny=8, nz=8, min_weight=1.0, workspace=P, totals=P, stream=None)
# mf_tsdfmesh_emit(volume, nx, ny, nz, ox, oy, oz, pitch, min_weight, workspace, n_vertices, n_faces, vertices, faces,
#                  normals, stream)
EMIT = dict(volume=P, nx=8, ny=8, nz=8, ox=0.0, oy=0.0, oz=0.0, pitch=0.1, min_weight=1.0, workspace=P, n_vertices=10,
            n_faces=10, vertices=P, faces=P, normals=None, stream=None)
NAN = float("nan")
BAD_DIMS = [dict(nx=1), dict(ny=1), dict(nz=0), dict(nx=-4), dict(nx=2048, ny=1024, nz=1024)]
BAD_WEIGHT = [dict(min_weight=0.0), dict(min_weight=-1.0), dict(min_weight=NAN)]


def _call(name, base, **change):
    L = mf._lib.lib()
    rc = getattr(L, name)(*dict(base, **change).values())
    return rc, L.mf_last_error_string()


@pytest.mark.parametrize("change", BAD_DIMS, ids=str)
def test_workspace_bytes_refuses(change):
    dims = dict(dict(nx=8, ny=8, nz=8), **change)
    assert mf._lib.lib().mf_tsdfmesh_workspace_bytes(*dims.values()) < 0


def test_workspace_bytes_of_the_largest_volume():
    n = 2047 * 1024 * 1024
    assert mf._lib.lib().mf_tsdfmesh_workspace_bytes(2047, 1024, 1024) == 2 * n + (1024 * 1024 + 1) * 16


@pytest.mark.parametrize("change", BAD_DIMS + BAD_WEIGHT + [
    dict(volume=None), dict(workspace=None), dict(totals=None), dict(volume=P + 8), dict(workspace=P + 4)], ids=str)
def test_count_refuses(change):
    rc, msg = _call("mf_tsdfmesh_count", COUNT, **change)
    assert rc == INVALID and b"mf_tsdfmesh_count" in msg


@pytest.mark.parametrize("change", BAD_DIMS + BAD_WEIGHT + [
    dict(pitch=0.0), dict(pitch=-0.1), dict(pitch=NAN), dict(n_vertices=-1), dict(n_faces=-1),
    dict(n_vertices=1 << 31), dict(n_faces=1 << 31), dict(volume=None), dict(workspace=None), dict(vertices=None),
    dict(faces=None), dict(volume=P + 8), dict(workspace=P + 4)], ids=str)
def test_emit_refuses(change):
    rc, msg = _call("mf_tsdfmesh_emit", EMIT, **change)
    assert rc == INVALID and b"mf_tsdfmesh_emit" in msg


def test_the_largest_allowed_scalars_reach_the_null_array_check():
    rc, msg = _call("mf_tsdfmesh_count", COUNT, nx=2047, ny=1024, nz=1024, volume=None, workspace=None, totals=None)
    assert rc == INVALID and b"null" in msg
    rc, msg = _call("mf_tsdfmesh_emit", EMIT, nx=2047, ny=1024, nz=1024, n_vertices=(1 << 31) - 1,
                    n_faces=(1 << 31) - 1, volume=None, workspace=None, vertices=None, faces=None)
    assert rc == INVALID and b"null" in msg

"""csrc/occserver.hip (with csrc/occmap.hip) through the host emulator behind contrib.OctomapServer (torch CPU tensors
as device memory), bit for bit against the mirror tests/occserver_ref.py: 48 x 64 frames of 3 objects on a table
(tests/occserver_cases.py).  Sequence A: three camera poses, the maps, centres and boxes after every frame.
Sequence B: one frame five times (cells reach the clamp), then the published grids under the four combinations of the
two no-entry flags, with the scene's branch counts asserted on the mirror alone."""
import numpy as np
import pytest

import occserver_cases as C
from host_emul import emul

pytestmark = pytest.mark.skipif(not emul.available(), reason="g++ not available")

H, W, N_OBJECTS, RESOLUTION = 48, 64, 3, 0.02


@pytest.fixture(scope="module")
def frames():
    return C.make_frames(0, H, W, N_OBJECTS)


@pytest.fixture()
def product(monkeypatch):
    emul.patch_lib(emul.build(["occmap.hip", "occserver.hip"]), monkeypatch)


def test_sequence_a_three_poses_bitwise(frames, product):
    assert not np.array_equal(frames[0]["T_sensor_to_map"], frames[1]["T_sensor_to_map"])
    assert (frames[0]["label"][::2, ::2] == -2).any() and (frames[0]["label"][::2, ::2] == C.LONE).sum() == 1
    C.run_sequence(frames, C.make_pitch_of(W), "cpu", RESOLUTION)


def test_sequence_b_clamped_cells_and_published_grids(frames, product):
    server, ref = C.run_clamped(frames[0], C.make_pitch_of(W), "cpu", RESOLUTION)
    C.check_clean(server)
    for ground in (True, False):
        for free in (True, False):
            C.check_publish(server, ref, frames[1]["T_sensor_to_map"], ground, free)


def test_scene_condition_objects_close_and_table_at_zero(frames):
    """Two objects within 16 voxels of each other; points of the table top at map z = 0."""
    import occserver_ref as S
    f, pitch_of = frames[0], C.make_pitch_of(W)
    ref = S.OctomapServer(resolution=RESOLUTION)
    C.insert(ref, f, pitch_of)
    ids = sorted(i for i in ref.centers if i not in (S.BACKGROUND_ID, C.LONE))
    near = [np.abs(ref.centers[a] - ref.centers[b]).max() / ref.octrees[a].resolution for a in ids for b in ids if a != b]
    assert min(near) < 16
    z = f["pts_map"][..., 2][f["label"] == -1]
    assert (np.abs(z[~np.isnan(z)]) < 1e-5).any()

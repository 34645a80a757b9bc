"""geometry.save_obj / load_obj with vertex colours (``v x y z r g b``), without a GPU: the round trip, a file without
colours, a file where only some vertices have one, and the default calls, which are what they were."""
import numpy as np
import pytest
import torch

from morefusion_amd import geometry

V = np.array([[0.1, 0.2, 0.3], [1.0, 0.0, -1.0 / 3.0], [0.0, 1e-17, 2.5], [4.0, 5.0, 6.0]])
F = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
RGBA = np.array([[255, 0, 10, 255], [1, 2, 3, 255], [200, 100, 50, 0], [128, 128, 128, 255]], np.uint8)


def test_round_trip_with_colours(tmp_path):
    path = str(tmp_path / "c.obj")
    geometry.save_obj(path, V, F, colors=RGBA)
    v, f, c = geometry.load_obj(path, return_colors=True)
    assert np.array_equal(v, V) and np.array_equal(f, F) and f.dtype == np.int32
    expected = RGBA[:, :3].astype(np.float64) / 255.0
    expected[2] = 0.0  # alpha 0: no colour was fused there
    assert c.dtype == np.float64 and c.shape == (4, 3) and np.array_equal(c, expected)
    assert np.array_equal(np.rint(c * 255.0).astype(np.uint8)[[0, 1, 3]], RGBA[[0, 1, 3], :3])
    lines = open(path).read().splitlines()
    assert [len(line.split()) for line in lines] == [7] * 4 + [4] * 2
    assert lines[0] == f"v {0.1:.17g} {0.2:.17g} {0.3:.17g} 1 0 {10 / 255:.17g}" and lines[2].endswith(" 0 0 0")


def test_tensors_and_three_channel_colours(tmp_path):
    path = str(tmp_path / "t.obj")
    geometry.save_obj(path, torch.as_tensor(V), torch.as_tensor(F), colors=torch.as_tensor(RGBA[:, :3]))
    v, f, c = geometry.load_obj(path, return_colors=True)
    assert np.array_equal(v, V) and np.array_equal(f, F)
    assert np.array_equal(c, RGBA[:, :3].astype(np.float64) / 255.0)  # no alpha: every colour is written


def test_bad_colours_are_refused(tmp_path):
    path = str(tmp_path / "bad.obj")
    for colors in (RGBA.astype(np.float32), RGBA[:3], RGBA[:, :2], RGBA.reshape(-1)):
        with pytest.raises(ValueError, match="colors must be uint8"):
            geometry.save_obj(path, V, F, colors=colors)


def test_a_file_without_colours(tmp_path):
    path = str(tmp_path / "plain.obj")
    geometry.save_obj(path, V, F)
    assert [len(line.split()) for line in open(path).read().splitlines()] == [4] * 6
    v, f, c = geometry.load_obj(path, return_colors=True)
    assert np.array_equal(v, V) and np.array_equal(f, F) and c is None


def test_a_file_where_some_vertices_have_a_colour(tmp_path):
    path = tmp_path / "some.obj"
    path.write_text("v 0 0 0\nv 1 0 0 0.5 0.25 1\nv 0 1 0 0.5\nf 1 2 3\n")
    v, f, c = geometry.load_obj(str(path), return_colors=True)
    assert v.shape == (3, 3) and f.tolist() == [[0, 1, 2]]
    assert np.array_equal(c, [[0, 0, 0], [0.5, 0.25, 1.0], [0, 0, 0]])


def test_the_default_calls_are_unchanged(tmp_path):
    """load_obj(path) returns the pair it returned before, also for a coloured file; save_obj without colours writes
    the bytes it wrote before."""
    coloured, plain = str(tmp_path / "c.obj"), str(tmp_path / "p.obj")
    geometry.save_obj(coloured, V, F, colors=RGBA)
    geometry.save_obj(plain, V, F)
    for path in (coloured, plain):
        out = geometry.load_obj(path)
        assert isinstance(out, tuple) and len(out) == 2
        assert np.array_equal(out[0], V) and out[0].dtype == np.float64
        assert np.array_equal(out[1], F) and out[1].dtype == np.int32
    expected = "".join(f"v {x:.17g} {y:.17g} {z:.17g}\n" for x, y, z in V.tolist()) + "f 1 2 3\nf 1 3 4\n"
    assert open(plain).read() == expected

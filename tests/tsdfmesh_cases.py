"""TEST INFRASTRUCTURE: the TSDF-mesh cases and their two runners -- the product (contrib.TsdfVolume.extract_mesh on a
device, or on the host emulator) and the mirror (tests/tsdfmesh_ref.py) -- whose vertices, faces and normals the tests
compare with array_equal.  A case is dict(volume float32 [nz, ny, nx, 2], pitch, origin).  The smallest shapes that can
still go wrong:
  a  the 23 x 19 x 17 volume of tsdf_cases.make_case("a") after its two integrates: fused data with unobserved
     regions, an open mesh; min_weight 1 and 2.
  b  an analytic sphere in 11 x 10 x 9: R = 2.6 pitches, the centre off the lattice, truncation 2 pitches (> sqrt(3)),
     weight 1 everywhere: closed, so welding, orientation and accuracy can be stated exactly.
  c  all 256 corner patterns in 2 x 2 x 767: pattern m in the layers 3 m and 3 m + 1, a weight-0 layer at 3 m + 2.
  d  300 x 3 x 3 with a tilted plane and two unobserved points: rows longer than a workgroup (ranks carried across
     waves and across the 256-column chunks of a row).
  e  7 x 4 x 5: tsdf alternating +0.5 / -0.5 along x (every central difference is 0: zero normals), an exact 0.0 and a
     -0.0 at corners (inside, r = 0 or 1, degenerate triangles) and an unobserved point (one-sided differences).
  f  a fresh volume and a fully positive observed one: no surface.
FULL_VOLUME with one 480 x 640 frame is the device's larger case and the end-to-end check (python
tests/tsdfmesh_cases.py prints what the two mirrors give for it).
"""
import numpy as np
import torch

import tsdf_cases as TC
import tsdf_ref as TR
import tsdfmesh_ref as R
from morefusion_amd import _lib
from morefusion_amd.contrib import TsdfVolume

FULL_VOLUME = dict(dims=(64, 64, 64), pitch=0.025, origin=(-0.8, -0.9, 0.2))  # that of tests/test_gpu_tsdf.py

SPHERE = dict(dims=(11, 10, 9), pitch=0.05, origin=(0.1, -0.2, 0.3), centre_index=(5.2, 4.6, 4.1), radius=2.6,
              truncation=2.0)  # centre, radius and truncation in pitches


def sphere_centre():
    return np.asarray(SPHERE["origin"], np.float64) + SPHERE["pitch"] * np.asarray(SPHERE["centre_index"], np.float64)


def _lattice(dims):
    nx, ny, nz = dims
    k, j, i = np.meshgrid(np.arange(nz, dtype=np.float64), np.arange(ny, dtype=np.float64),
                          np.arange(nx, dtype=np.float64), indexing="ij")
    return i, j, k


def _pack(F, W):
    return np.ascontiguousarray(np.stack([np.asarray(F, np.float32), np.asarray(W, np.float32)], -1))


def make_case(name):
    if name == "a":
        case = TC.make_case("a")
        v = case["volume"]
        return dict(volume=TC.run_mirror(case)[1]["volume"], pitch=v["pitch"], origin=v["origin"])
    if name == "b":
        h, (i, j, k) = SPHERE["pitch"], _lattice(SPHERE["dims"])
        c, o = sphere_centre(), SPHERE["origin"]
        dist = np.sqrt(((o[0] + h * i) - c[0]) ** 2 + ((o[1] + h * j) - c[1]) ** 2 + ((o[2] + h * k) - c[2]) ** 2)
        F = np.clip((dist - SPHERE["radius"] * h) / (SPHERE["truncation"] * h), -1.0, 1.0)
        return dict(volume=_pack(F, np.ones_like(F)), pitch=h, origin=o)
    if name == "c":
        F, W = np.ones((767, 2, 2), np.float32), np.zeros((767, 2, 2), np.float32)
        for m in range(256):
            for code in range(8):
                dx, dy, dz = code >> 2, (code >> 1) & 1, code & 1
                # different magnitudes at every corner: the vertices are not midpoints
                F[3 * m + dz, dy, dx] = -(0.2 + 0.05 * code) if m >> code & 1 else 0.3 + 0.05 * code
            W[3 * m:3 * m + 2] = 1.0
        return dict(volume=_pack(F, W), pitch=0.02, origin=(0.0, 0.0, 0.0))
    if name == "d":
        i, j, k = _lattice((300, 3, 3))
        # the rows (j, k) cross zero at i = 11 .. 322: the row (1, 0) between columns 255 and 256
        F = np.clip(((0.009 * i + 0.6 * j + 0.8 * k) - 2.9) / 2.0, -1.0, 1.0)
        W = np.full(F.shape, 3.0)
        W[1, 1, 100], W[0, 2, 257] = 0.0, 0.5
        return dict(volume=_pack(F, W), pitch=0.01, origin=(-1.5, 0.0, 0.4))
    if name == "e":
        i, j, k = _lattice((7, 4, 5))
        F = np.where(i % 2 == 0, 0.5, -0.5).astype(np.float32)
        F[1, 1, 2], F[2, 2, 4] = 0.0, -0.0
        W = np.ones(F.shape, np.float32)
        W[0, 0, 4] = 0.0
        return dict(volume=_pack(F, W), pitch=0.1, origin=(0.0, 0.0, 0.0))
    if name == "f_fresh":
        return dict(volume=TR.fresh((5, 4, 3)), pitch=0.1, origin=(0.0, 0.0, 0.0))
    if name == "f_positive":
        F = np.full((3, 4, 5), 0.7, np.float32)
        return dict(volume=_pack(F, np.ones_like(F)), pitch=0.1, origin=(0.0, 0.0, 0.0))
    raise KeyError(name)


NAMES = ("a", "b", "c", "d", "e", "f_fresh", "f_positive")


def run_mirror(case, min_weight=1.0):
    return R.mesh(case["volume"], case["origin"], case["pitch"], min_weight)


def volume_of(case, device):
    nz, ny, nx = case["volume"].shape[:3]
    vol = TsdfVolume((nx, ny, nz), case["pitch"], case["origin"], device=device)
    vol.volume.copy_(torch.from_numpy(case["volume"]))
    return vol


def run_product(case, device, min_weight=1.0):
    """-> dict(vertices, faces, normals) as NumPy; the call without normals must give the same vertices and faces."""
    vol = volume_of(case, device)
    v, f, n = vol.extract_mesh(min_weight=min_weight, normals=True)
    v2, f2 = vol.extract_mesh(min_weight=min_weight)
    for t, dtype in ((v, torch.float64), (f, torch.int32), (n, torch.float64), (v2, torch.float64), (f2, torch.int32)):
        assert t.dtype == dtype and t.device == vol.volume.device and t.dim() == 2 and t.shape[1] == 3
    assert torch.equal(v, v2) and torch.equal(f, f2)
    return dict(vertices=v.cpu().numpy(), faces=f.cpu().numpy(), normals=n.cpu().numpy())


def assert_equal(got, exp):
    for key in ("vertices", "faces", "normals"):
        g, e = got[key], exp[key]
        assert g.dtype == e.dtype and g.shape == e.shape, (key, g.shape, e.shape)
        # array_equal on the bits: -0.0 and 0.0 differ, a NaN equals itself
        assert g.tobytes() == e.tobytes(), (key, int((g != e).sum()))


class CountingLib:
    """A proxy of the library that counts the calls of every entry point."""

    def __init__(self, lib):
        self._lib, self.calls = lib, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*args)
        return call


def full_volume_mirror(frames):
    """FULL_VOLUME after frame 0 of ``frames`` -> (the case, the mirror's tsdf volume)."""
    ref = TR.Volume(**FULL_VOLUME)
    ref.integrate(frames[0]["depth"], frames[0]["K"], frames[0]["T_sensor_to_map"])
    return dict(volume=ref.volume, pitch=FULL_VOLUME["pitch"], origin=FULL_VOLUME["origin"]), ref


if __name__ == "__main__":
    import camtrack_cases as CC
    import render_ref
    frames = CC.sequence(0, 2, 480, 640)
    case, ref = full_volume_mirror(frames)
    m = run_mirror(case)
    T1 = frames[1]["T_sensor_to_map"]
    ray, code = ref.raycast(frames[0]["K"], T1, 480, 640)
    out = render_ref.render([(m["vertices"], m["faces"])], [np.linalg.inv(T1)], frames[0]["K"], 480, 640)
    depth = out["depth"][0]
    both = (code == TR.HIT) & ~np.isnan(depth)
    print("vertices", len(m["vertices"]), "faces", len(m["faces"]), "pixels with both", int(both.sum()),
          "median |render - raycast| / pitch", float(np.median(np.abs(depth[both] - ray[both]))) / FULL_VOLUME["pitch"])

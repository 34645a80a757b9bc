"""The fp32 3-D inference kernels' TEXT (csrc/linear.hip, conv3d.hip, sparseconv.hip, interp.hip, pointops.hip) on the
host emulator, through the C ABI, on the cases of tests/volumetric_fp32_cases.py (its docstring says which case reaches
which branch) against the float64 references, mirrors and the a-priori bound of tests/volumetric_fp32_ref.py.  Every
output element is compared; every "device" buffer ends at an inaccessible page (``emul.guarded``), outputs are
sentinel-filled and embedded.  The comparator itself is shown to reject the errors a plausible kernel bug would make,
on NumPy arrays only (the project's code is never broken to show that a test bites)."""
import numpy as np
import pytest

import volumetric_fp32_cases as C
import volumetric_fp32_ref as R
from host_emul import emul

pytestmark = pytest.mark.skipif(not emul.available(), reason="g++ not available")


class Guarded(C.Host):
    """``Host`` whose buffers end right in front of an inaccessible page (16-byte sized ones: the aligned kernels need
    the start aligned too)."""
    @staticmethod
    def dev(a):
        a = np.ascontiguousarray(a)
        return emul.guarded(a) if a.nbytes and a.nbytes % 16 == 0 else a.copy()


X = Guarded


@pytest.fixture(scope="module")
def lin_lib():
    return emul.build(["linear.hip"])


@pytest.fixture(scope="module")
def conv_lib():
    return emul.build(["conv3d.hip"])


@pytest.fixture(scope="module")
def sc_lib():
    return emul.build(["sparseconv.hip"])


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    C.report()


def _maybe_skip(key):
    if key in C.EMUL_SKIP:
        pytest.skip("left out on the emulator (volumetric_fp32_cases.EMUL_SKIP): " + C.EMUL_SKIP[key])


@pytest.mark.parametrize("name", list(C.LINEAR))
def test_linear_every_element_within_its_bound(lin_lib, name):
    _maybe_skip("linear " + name)
    C.check_linear(name, C.run_linear(lin_lib, X, name), "emul")


def test_linear_cases_reach_both_tile_heights_with_and_without_the_remap():
    grids = {n: C.linear_grid(c) for n, c in C.LINEAR.items()}
    assert grids["mi2_grid264"] == (2, 264) and grids["mi2_grid273"] == (2, 273)
    assert grids["mi1_grid8"] == (1, 8) and grids["mi1_grid6"] == (1, 6)
    assert all(g[0] == 1 and g[1] % 8 for n, g in grids.items() if not n.startswith("mi"))


def test_linear_refusals(lin_lib):
    C.check_linear_refusals(lin_lib, X)


@pytest.mark.parametrize("name", list(C.CONV))
def test_conv3d_k4s2_every_element_within_its_bound(conv_lib, name):
    _maybe_skip("conv " + name)
    got = C.run_conv(conv_lib, X, name)
    C.check_conv(name, got, "emul")
    if C.CONV[name]["split"] == "max":
        C.bits_equal(C.run_conv(conv_lib, X, name)["out"], got["out"], f"conv {name}: a second launch")


def test_conv3d_refusals(conv_lib):
    C.check_conv_refusals(conv_lib, X)


@pytest.mark.parametrize("name", list(C.OCC))
def test_occupancy_convs_every_element_within_its_bound(conv_lib, name):
    C.check_occ(name, C.run_occ(conv_lib, X, name), "emul")


@pytest.mark.parametrize("shape", C.TCL)
def test_to_channels_last_bits(conv_lib, shape):
    C.run_check_tcl(conv_lib, X, shape, "emul")


@pytest.mark.parametrize("name", list(C.SPARSE))
def test_sparse_conv3_every_entry_within_its_bound_and_bit_equal(sc_lib, name):
    C.check_sparse(sc_lib, X, name, "emul")


@pytest.mark.parametrize("shape", C.INTERP)
def test_interpolate_channels_last_bits(shape):
    C.run_check_interp(emul.build(["interp.hip"]), X, shape, "emul")


@pytest.mark.parametrize("shape", C.PREP)
def test_point_prep_bits_and_pose_epilogue_within_its_bound(shape):
    C.run_check_prep(emul.build(["pointops.hip"]), X, shape, "emul")


# ---- the comparator bites: plausible kernel bugs, applied to the REFERENCE's own output -------------------------------
def test_comparator_accepts_the_reference_and_rejects_plausible_corruptions():
    name = "m63_k32_n63"
    c = C.LINEAR[name]
    A, W, b = C.linear_data(name)
    ref, S, K = R.linear(A[:, :32], W[0, :128 * 32].reshape(128, 32)[:63], None, 0)
    out = np.full((c["M"] + 2, c["ldo"]), C.SENT, np.float32)
    out[1:64, 4:67] = ref
    C.check_linear(name, out, "self")
    # the last chunk of K dropped (``<`` for ``<=`` in the K guard)
    bad = out.copy()
    bad[1:64, 4:67] = R.linear(A[:, :28], W[0, :128 * 32].reshape(128, 32)[:63, :28], None, 0)[0]
    with pytest.raises(AssertionError, match="linear"):
        C.check_linear(name, bad, "corrupt")
    # a 16-byte store over the end of the block (column N), and a row left unwritten
    bad = out.copy()
    bad[1, 67] = 0.25
    with pytest.raises(AssertionError, match="outside"):
        C.check_linear(name, bad, "corrupt")
    bad = out.copy()
    bad[63, 4:67] = C.SENT
    with pytest.raises(AssertionError, match="unwritten"):
        C.check_linear(name, bad, "corrupt")
    # one wrong element beside large ones: a max-norm tolerance of 1e-4 max|ref| passes it, the bound does not
    i = np.unravel_index(np.argmin(S), S.shape)
    bad = out.copy()
    bad[1 + i[0], 4 + i[1]] += 5e-5 * np.abs(ref).max()
    assert 5e-5 * np.abs(ref).max() > 2 * K * R.U32 * S[i]
    with pytest.raises(AssertionError, match="linear"):
        C.check_linear(name, bad, "corrupt")
    # S == 0 must be exact
    r, _, _ = R.ratios(np.array([1e-30]), np.array([0.0]), np.array([0.0]), 8)
    assert np.isinf(r[0])

"""The specialised forms of the ICC iteration kernels on the MI355X (k_icc_fused3<MAXNS>)
against the kernels that carry every case, bit for bit, and against the oracle.  Three fresh child processes run every
case of tests/icc_specialised_ref.py once: the default (auto), MF_ICC_FUSED_FORM=generic, and the default again."""
import os
import subprocess
import sys

import numpy as np
import pytest

import icc_specialised_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    out = {}
    d = tmp_path_factory.mktemp("icc_specialised")
    for tag, form in (("auto", None), ("generic", "generic"), ("auto_again", None)):
        env = {k: v for k, v in os.environ.items() if k not in ("MF_ICC_FUSED_FORM", "MF_ICC_BIN_CAP", "MF_ICC_GENERAL")}
        if form:
            env["MF_ICC_FUSED_FORM"] = form
        path = str(d / f"{tag}.npz")
        subprocess.run([sys.executable, os.path.join(ROOT, "tests", "icc_specialised_ref.py"), path], env=env, cwd=ROOT,
                       check=True, timeout=300)
        z = np.load(path)
        out[tag] = {name: {k: z[f"{name}/{k}"] for k in R.KEYS + ("form",)} for name in R.CASES}
    return out


@pytest.mark.parametrize("name", list(R.CASES))
def test_specialised_forms_give_the_fall_backs_bits_and_the_oracles_steps(runs, name):
    auto, generic, again = (runs[k][name] for k in ("auto", "generic", "auto_again"))
    assert int(auto["form"]) == R.CASES[name]["form"], auto["form"]     # the library that ran planned this form
    assert int(generic["form"]) == R.GENERIC
    R.check_bitwise(auto, generic, "auto against MF_ICC_FUSED_FORM=generic")      # (i)
    R.check_vs_oracle(name, auto)                                                # (ii)
    R.check_bitwise(auto, again, "two runs of auto")                             # (iii)

"""The Adam/Polyak kernels against bits recorded from the kernels they
replaced (tests/golden/adam_family.npz, written by
tools/record_adam_golden.py on the commit before the kernels were folded
into k_adam_groups).

The other bit-equality tests of this family compare one path through the
shared element update with another; this one pins all of them to an
anchor outside the code under test.  Every array any case writes is
compared after every step with torch.equal on its bits (fp32 as int32,
bf16 as int16), so the sign of zero and the payload of a NaN count too.
"""

import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["c1", "c2_1", "c2_257", "c2_1000", "c3", "c4", "c5", "c6",
         "c7_tau", "c7_one"]


def _recorder():
    spec = importlib.util.spec_from_file_location(
        "record_adam_golden",
        os.path.join(REPO, "tools", "record_adam_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def replay():
    """(recorded, replayed): {name: bit view} of every output array."""
    from distributed_sac_amd.ops import native
    rec = _recorder()
    with np.load(rec.GOLDEN) as z:
        inp = {k[3:]: torch.from_numpy(z[k]) for k in z.files
               if k.startswith("in/")}
        want = {k[4:]: torch.from_numpy(z[k]) for k in z.files
                if k.startswith("out/")}
    got = {k: rec.bits(v) for k, v in rec.run_cases(native(), inp).items()}
    return {k: rec.bits(v) for k, v in want.items()}, got


def test_fixture_covers_every_case(replay):
    want, got = replay
    assert sorted(want) == sorted(got)
    assert {k.split("/")[0] for k in want} == set(CASES)


@pytest.mark.parametrize("case", CASES)
def test_adam_family_matches_recorded_bits(replay, case):
    want, got = replay
    keys = sorted(k for k in want if k.split("/")[0] == case)
    assert keys
    bad = [f"{k}: {int((got[k] != want[k]).sum())} of {want[k].numel()}"
           for k in keys
           if got[k].dtype != want[k].dtype or got[k].shape != want[k].shape
           or not torch.equal(got[k], want[k])]
    assert not bad, bad

"""Every fused rollout-timestep entry against what it wrote at the commit before the timestep's shared pieces moved
into csrc/rollout_step.hip.h: bit for bit, every output buffer, no tolerance.  The cases and their closed-form inputs
are tests/golden/generate_rollout_step_fixtures.py's, which also recorded tests/golden/rollout_step_parity.npz."""

import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location(
    "generate_rollout_step_fixtures",
    os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "generate_rollout_step_fixtures.py"))
fixtures = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(fixtures)


def test_the_fixture_holds_every_case_and_nothing_else(golden):
    recorded = {key.rsplit("/", 1)[0] for key in golden("rollout_step_parity.npz")}
    assert recorded == {fixtures.case_id(*case) for case in fixtures.CASES} and len(recorded) == 11 * 3 * 3 * 2


@pytest.mark.parametrize("entry,n,mode,rdr", fixtures.CASES, ids=[fixtures.case_id(*case) for case in fixtures.CASES])
def test_rollout_step_writes_what_the_parent_commit_wrote(golden, entry, n, mode, rdr):
    want = golden("rollout_step_parity.npz")
    prefix = fixtures.case_id(entry, n, mode, rdr) + "/"
    got = fixtures.run_case(entry, n, mode, rdr)
    assert {prefix + name for name in got} == {key for key in want if key.startswith(prefix)}
    for name, array in got.items():
        assert array.dtype == want[prefix + name].dtype and np.array_equal(array, want[prefix + name]), name

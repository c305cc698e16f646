"""The host planners of the ragged calls write, for every case of the ragged fixtures and a handful of bad inputs each, exactly the
bytes, workspace sizes and return codes recorded in tests/golden/many_plans.json (made by tests/golden/make_golden_many_plans.py with
an earlier commit's library; which one is in its docstring).  No GPU: a plan is host arithmetic."""
import hashlib
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import kit_golden  # noqa: E402
import many_plan_cases  # noqa: E402

with open(os.path.join(kit_golden.GOLDEN, "many_plans.json")) as _f:
    FROZEN = json.load(_f)
GROUPS = sorted({k.split("/")[0] for k in FROZEN})


@pytest.fixture(scope="module")
def planned():
    return {key: [rc, ws, hashlib.sha256(block).hexdigest()] for key, rc, ws, block in many_plan_cases.plans()}


def test_the_key_set_is_complete(planned):
    assert sorted(planned) == sorted(FROZEN)
    assert GROUPS == ["alpha", "back", "back_bwd", "embed", "err", "many", "maps", "merged", "nearest", "patches", "placed", "reduce", "ycbcr"]
    assert {k.split("/")[1] for k in FROZEN if k.startswith("err/")} == {"many", "patches", "nearest", "reduce", "maps", "ycbcr", "embed", "back",
                                                                         "merged", "back_bwd"}


@pytest.mark.parametrize("group", GROUPS)
def test_every_plan_is_the_frozen_one(planned, group):
    keys = [k for k in FROZEN if k.startswith(group + "/")]
    assert keys
    assert all(FROZEN[k][0] == 0 for k in keys) or group == "err"  # every fixture case plans; only the literal bad inputs fail
    different = {k: (planned[k], FROZEN[k]) for k in keys if planned[k] != FROZEN[k]}
    assert not different, f"{len(different)} of {len(keys)} plans differ, the first: {sorted(different.items())[0]}"

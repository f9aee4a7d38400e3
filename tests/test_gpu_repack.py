"""The load-time repack on the device == the golden tiles, bit for bit.

The engine always repacks with device="cuda"; the CPU tests run the same
torch code with "cpu". This asserts the device run of every golden case
(tests/repack_cases.py) produces the recorded bytes, i.e. that the two
agree.
"""
import pytest

import repack_cases as RC
from distributedllm_amd.engine.repack import repack_mfma

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("group", RC.GROUPS)
def test_device_repack_matches_golden(group):
    cases = RC.cases(group)
    assert cases
    for case_id, t in cases:
        data, scales, wtype = repack_mfma(t, "cuda")
        assert data.is_cuda
        RC.check(case_id, t, (data, scales, wtype))

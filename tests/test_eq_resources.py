"""Resource budgets of the equaliser's kernels, read from the code objects inside libconan_hip.so: no scratch, no spills, and at most
64 KB of LDS - one workgroup of 256 lanes per row that does not wait for a whole CU beside the vocoder."""
import pytest

from tests.test_kernel_resources import _find, _kernels


@pytest.mark.parametrize("name", ["eq_signal_kernel", "eq_stream_kernel", "eq_set_kernel", "eq_state_kernel"])
def test_eq_kernels_stay_small(tmp_path, name):
    k = _find(_kernels(tmp_path), name)
    assert k["scratch"] == 0 and k["spill"] == 0, (name, k)
    assert k["lds"] <= 64 * 1024, (name, k)

"""ncclAllReduceWithBias without a GPU: both names are exported and refuse a NULL comm as ncclAllReduce does."""
import ctypes

import pytest

from vccl_amd import nccl


@pytest.mark.parametrize("prefix,acc", [(p, a) for p in ("", "p") for a in (None, 16)])
def test_null_comm(prefix, acc):
    args = (ctypes.c_void_p(0x10), ctypes.c_void_p(0x20), ctypes.c_size_t(4), 7, 0, None, None, ctypes.c_void_p(acc))
    assert getattr(nccl.lib(), prefix + "ncclAllReduceWithBias")(*args) == nccl.ncclInvalidArgument

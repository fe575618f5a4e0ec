"""CPU tests of the registration table behind ncclCommRegister (host/reg.cc,
through vcclRegTable*): lookup of an interior pointer plus length, two ranges
in one allocation, overlap, removal, generations, capacity.  No GPU needed."""
import ctypes

import pytest

from vccl_amd import nccl

BASE = 0x7F00_0000_0000


@pytest.fixture
def table():
    t = nccl.RegTable()
    yield t
    t.free()


def test_interior_pointer_and_length(table):
    e, g = table.insert(BASE + 256, 4096)
    assert (e, g) == (0, 1)
    assert table.find(BASE + 256, 4096) == (0, 0, 1)             # the whole range
    assert table.find(BASE + 256 + 100, 1000) == (0, 100, 1)     # inside
    assert table.find(BASE + 256 + 100, 4096 - 100) == (0, 100, 1)   # touching the end
    assert table.find(BASE + 256 + 100, 4096 - 99)[0] == -1      # one byte over
    assert table.find(BASE + 255, 2)[0] == -1                    # one byte before
    assert table.find(BASE + 256 + 4095, 1) == (0, 4095, 1)
    assert table.find(BASE + 256 + 4096, 0)[0] == -1             # the end itself is outside
    assert table.find(BASE + 256 + 4096, 1)[0] == -1
    assert table.find(BASE + 300, 0) == (0, 44, 1)
    assert table.find((1 << 64) - 8, 16)[0] == -1                # a range that wraps is nowhere


def test_two_ranges_in_one_allocation(table):
    a, _ = table.insert(BASE, 1000)
    b, _ = table.insert(BASE + 2000, 1000)
    assert (a, b) == (0, 1)
    assert table.find(BASE + 10, 100)[:2] == (0, 10)
    assert table.find(BASE + 2010, 100)[:2] == (1, 10)
    assert table.find(BASE + 1500, 10)[0] == -1          # the gap
    assert table.find(BASE + 900, 1200)[0] == -1         # spans the gap
    # adjacent ranges: their union is not one registration
    c, _ = table.insert(BASE + 1000, 1000)
    assert c == 2 and table.find(BASE + 900, 200)[0] == -1
    assert table.find(BASE + 1000, 1000)[:2] == (2, 0)


def test_overlap(table):
    """Overlapping and repeated registrations are entries of their own; a
    lookup gives the lowest live entry that holds the whole range."""
    assert table.insert(BASE, 1000)[0] == 0
    assert table.insert(BASE + 500, 1000)[0] == 1
    assert table.insert(BASE, 1000)[0] == 2              # the same range again: its own handle
    assert table.find(BASE + 600, 100)[:2] == (0, 600)   # both hold it: the lowest
    assert table.find(BASE + 600, 600)[:2] == (1, 100)   # only the second holds it
    assert table.find(BASE + 100, 1300)[0] == -1         # only their union would
    assert table.remove(0) == nccl.ncclSuccess
    assert table.find(BASE + 600, 100)[:2] == (1, 100)
    assert table.find(BASE + 100, 100)[:2] == (2, 100)   # the repeat is still registered


def test_remove_then_find_and_generation(table):
    e, g = table.insert(BASE, 64)
    assert (e, g) == (0, 1)
    assert table.remove(0) == nccl.ncclSuccess
    assert table.find(BASE, 64)[0] == -1
    assert table.remove(0) == nccl.ncclInvalidArgument           # not live any more
    for bad in (-1, 32, 1 << 20):
        assert table.remove(bad) == nccl.ncclInvalidArgument
    # the entry is reused, under a generation no former occupant had
    e2, g2 = table.insert(BASE + 4096, 128)
    assert (e2, g2) == (0, 3)
    assert table.find(BASE + 4096, 128) == (0, 0, 3)
    assert table.find(BASE, 64)[0] == -1
    gens = {g, g2}
    for _ in range(50):
        assert table.remove(0) == nccl.ncclSuccess
        e3, g3 = table.insert(BASE, 64)
        assert e3 == 0 and g3 % 2 == 1 and g3 not in gens
        gens.add(g3)


def test_capacity(table):
    """The 33rd insert is refused without an error; a freed entry is handed out again."""
    for i in range(nccl.REG_MAX_ENTRIES):
        assert table.insert(BASE + i * 4096, 4096) == (i, 1)
    assert table.insert(BASE + 64 * 4096, 4096) == (-1, 0)
    assert table.find(BASE + 64 * 4096, 1)[0] == -1
    for i in range(nccl.REG_MAX_ENTRIES):
        assert table.find(BASE + i * 4096 + 7, 4089) == (i, 7, 1)
    assert table.remove(17) == nccl.ncclSuccess
    assert table.insert(BASE + 64 * 4096, 4096) == (17, 3)
    assert table.insert(BASE + 65 * 4096, 4096)[0] == -1
    # empty ranges are refused the same way
    assert table.remove(3) == nccl.ncclSuccess
    assert table.insert(BASE, 0)[0] == -1
    assert table.insert(BASE, 1)[0] == 3


def test_null_arguments():
    L = nccl.lib()
    e = ctypes.c_int()
    assert L.vcclRegTableNew(None) == nccl.ncclInvalidArgument
    assert L.vcclRegTableInsert(None, 1, 1, ctypes.byref(e), None) == nccl.ncclInvalidArgument
    assert L.vcclRegTableFind(None, 1, 1, ctypes.byref(e), None, None) == nccl.ncclInvalidArgument
    assert L.vcclRegTableRemove(None, 0) == nccl.ncclInvalidArgument
    assert L.vcclRegTableFree(None) == nccl.ncclSuccess
    t = nccl.RegTable()
    assert L.vcclRegTableInsert(t.handle, 1, 1, None, None) == nccl.ncclInvalidArgument
    t.free()

"""The payload generator (tests/_payloads.py) and the oracle on its payloads:

* hard_input is deterministic, lays the specials table where it says, and the
  table holds every class the payloads promise;
* the cap — NaNs at most 25 % of an expected output, and a finite non-zero,
  an infinite (fp8: saturated), a -0 and a subnormal element in every float
  one — for every (type, op, n) of the collective matrix on every path's
  expectation (the chain fold, the ring / LL / LL128 partitions' folds);
* the oracle's chain fold against an independent left fold of the same order
  (numpy; torch CPU bfloat16 for bf16 — the independence rule of
  tests/golden/gen_golden.py), bit-exact, so the oracle is validated on
  specials at every position of a stream, not only in a vector's first 14.
"""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import _payloads as P
from tests import ring_cases as RC
from tests._util import assert_bitexact

NCH, SLOT = 14, 256 << 10  # the collective tests' geometry


def _bits(a):
    return np.ascontiguousarray(a).view(P._UINT[a.dtype.itemsize])


def test_deterministic():
    for dt in P.MATRIX_TYPES + (1, 3, 4):
        for op in P.MATRIX_OPS:
            a = P.hard_input(dt, op, 1000, 1, 3, 7)
            b = P.hard_input(dt, op, 1000, 1, 3, 7)
            assert a.dtype == O.NP_DTYPE[dt] and a.size == 1000
            assert np.array_equal(_bits(a), _bits(b))
            for other in (P.hard_input(dt, op, 1000, 2, 3, 7), P.hard_input(dt, op, 1000, 1, 3, 8)):
                assert not np.array_equal(_bits(a), _bits(other))
            # a longer stream starts with the shorter one's specials, laid down as documented
            t = _bits(P.table(dt, op))
            pos = np.arange(1000)
            sp = pos % P.PERIOD < P.SPAN
            want = t[(pos[sp] % P.PERIOD + P.STRIDE * 1 + pos[sp] // P.PERIOD) % t.size]
            assert np.array_equal(_bits(a)[sp], want)
            assert sp.sum() == 61 * 3 + 61


@pytest.mark.parametrize("dt", sorted(P.FLOAT_FMT))
def test_float_table_classes(dt):
    e_bits, m = P.FLOAT_FMT[dt]
    s, expmask = 1 << (e_bits + m), ((1 << e_bits) - 1) << m
    quiet = 1 << (m - 1)
    for op in P.MATRIX_OPS:
        t = set(int(v) for v in _bits(P.table(dt, op)))
        assert len(P.table(dt, op)) <= 61
        for v in (0, s, expmask, s | expmask, 1, (1 << m) - 1, 1 << m, expmask - 1, s | (expmask - 1)):
            assert v in t, (dt, op, hex(v))
        nans = [v for v in t if v & (s - 1) > expmask]
        assert any(v & quiet and v & (quiet - 1) for v in nans)  # a quiet NaN with a payload
        assert any(not v & quiet for v in nans) == (op in (0, 1, 4))  # the signalling one: sum / prod / avg only
        # x / -x pairs and the two ties' operands
        one = ((1 << (e_bits - 1)) - 1) << m
        half_ulp = one - ((m + 1) << m)  # 2^-(m+1)
        assert {one, s | one, one | 1, half_ulp, expmask - 1 - (1 << m), s | (expmask - 1 - (1 << m))} <= t


@pytest.mark.parametrize("dt", P.F8_TYPES)
def test_fp8_table_classes(dt):
    t = set(int(v) for v in P.table(dt))
    c = P._F8[dt]
    assert {0x00, 0x80, 0x7c, 0xfc, c["maxf"], 0x80 | c["maxf"], c["maxsub"], c["minsub"]} <= t
    vals = O.fp8_bits_to_f32(dt, np.array(sorted(t), np.uint8))
    nan_codes = [v for v, f in zip(sorted(t), vals) if np.isnan(f)]
    assert any(v & 0x80 for v in nan_codes) and any(not v & 0x80 for v in nan_codes)
    f = lambda code: float(O.fp8_bits_to_f32(dt, np.array([code], np.uint8))[0])  # noqa: E731
    assert f(c["one"]) == 1.0 and f(c["half"]) == 0.5
    ulp = f(c["one_ulp"]) - 1.0
    assert f(c["ulp_half"]) == ulp / 2  # 1 + ulp/2 and (1 + ulp) + ulp/2: a tie of each parity
    assert f(c["minnorm"]) == f(c["maxsub"]) + f(c["minsub"])
    assert np.isinf(f(0x7c)) == (dt == 11)


@pytest.mark.parametrize("dt", P.INT_TYPES)
def test_int_table_classes(dt):
    info = np.iinfo(O.NP_DTYPE[dt])
    t = set(int(v) for v in P.table(dt))
    want = {info.min, info.max, 0, 1, info.min + 1}
    want |= {info.max // n + d for n in range(2, 9) for d in (-1, 1)}
    bits = info.bits
    for b in (0x7f, 0x80, 0xff):
        v = int.from_bytes(bytes([b]) * (bits // 8), "little")
        want.add(v - (1 << bits) if info.min and v > info.max else v)
    if info.min:
        want.add(-1)
    assert want <= t, sorted(want - t)


def test_pairs():
    a, b = P.all_pairs_u8()
    assert a.dtype == b.dtype == np.uint8 and a.size == b.size == 65536
    assert len(set(zip(a.tolist(), b.tolist()))) == 65536
    for dt in list(P.FLOAT_FMT) + list(P.F8_TYPES):
        for op in P.MATRIX_OPS:
            t = P.table(dt, op)
            x, y = P.special_pairs(dt, op)
            assert x.size == y.size == t.size ** 2
            assert np.array_equal(_bits(x.reshape(t.size, t.size)[:, 0]), _bits(t))
            assert np.array_equal(_bits(y[:t.size]), _bits(t))
            # the pairs' expected output keeps to the NaN bound as well
            dev_op, arg = O.host_to_dev_redop(op, dt, 2)
            pre = 2 if dev_op == O.DEV_PREMULSUM else 0
            exp = O.reduce_copy(dev_op, dt, arg, [x, y], pre_op_args=[arg] * pre)[0]
            assert 4 * P.classes(dt, exp)["nan"] <= exp.size, (dt, op)


def _inputs(dt, op, n, count):
    return [P.hard_input(dt, op, count, r, n, P.SEED) for r in range(n)]


@pytest.mark.parametrize("n", P.MATRIX_RANKS)
@pytest.mark.parametrize("dt", P.MATRIX_TYPES)
def test_cap_on_every_path(dt, n):
    """NaN share and class presence in what every path of the collective
    matrix is expected to produce (tests/test_gpu_payloads.py)."""
    for op in P.MATRIX_OPS:
        ar = _inputs(dt, op, n, P.AR_COUNT)
        rs = _inputs(dt, op, n, n * P.RS_COUNT)
        for path in ("ll", "ring", "ll128"):  # direct folds in the ring's order
            what = f"{O.TYPE_NAMES[dt]} {O.OP_NAMES[op]} n={n} {path}"
            P.assert_cap(dt, RC.expected_on_path(path, "ar", op, dt, ar, NCH, SLOT), "ar " + what)
            for r, e in enumerate(RC.expected_on_path(path, "rs", op, dt, rs, NCH, SLOT)):
                P.assert_cap(dt, e, f"rs rank {r} " + what)
            if path != "ll128":
                P.assert_cap(dt, RC.expected_on_path(path, "red", op, dt, ar, NCH, SLOT, root=n - 1), "red " + what)


# ------------------------------------------------ the independent left fold
def _to_torch_bf16(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16).copy()).view(torch.bfloat16)


def _left_fold(dt, op, srcs):
    """acc = pre(srcs[0]); acc = acc (+) pre(s) — never through the oracle."""
    n = len(srcs)
    if dt in P.INT_TYPES:
        npdt = np.dtype(O.NP_DTYPE[dt])
        with np.errstate(over="ignore"):
            acc = srcs[0].copy()
            for s in srcs[1:]:
                if op in (0, 4):
                    acc = (acc + s).astype(npdt)
                elif op == 1:
                    acc = (acc * s).astype(npdt)
                else:
                    acc = (np.maximum if op == 2 else np.minimum)(acc, s)
        if op == 4:  # SumPostDiv: the wrapped sum, divided truncating toward zero
            acc = np.array([(abs(x) // n) * (1 if x >= 0 else -1) for x in acc.tolist()], dtype=object).astype(npdt)
        return acc
    if dt == 9:
        xs = [_to_torch_bf16(s) for s in srcs]
        scal = torch.tensor(1.0 / n, dtype=torch.float32).to(torch.bfloat16)
        pre = (lambda x: x * scal) if op == 4 else (lambda x: x)
        acc = pre(xs[0])
        for s in xs[1:]:
            s = pre(s)
            acc = acc + s if op in (0, 4) else acc * s if op == 1 else torch.fmax(acc, s) if op == 2 \
                else torch.fmin(acc, s)
        return acc.view(torch.int16).numpy().view(np.uint16)
    npdt = O.NP_DTYPE[dt]
    scal = npdt(np.float32(1.0 / n)) if dt != 8 else 1.0 / n
    pre = (lambda x: (x * scal).astype(npdt)) if op == 4 else (lambda x: x)
    with np.errstate(all="ignore"):
        acc = pre(srcs[0])
        for s in srcs[1:]:
            s = pre(s)
            acc = (acc + s).astype(npdt) if op in (0, 4) else (acc * s).astype(npdt) if op == 1 \
                else np.fmax(acc, s) if op == 2 else np.fmin(acc, s)
    return acc


@pytest.mark.parametrize("n", [2, 3, 4])
@pytest.mark.parametrize("dt", [0, 1, 2, 3, 4, 5, 6, 7, 8, 9])
def test_oracle_chain_fold_vs_independent_fold(dt, n):
    for op in P.MATRIX_OPS:
        ins = _inputs(dt, op, n, P.AR_COUNT)
        dev_op, arg = O.host_to_dev_redop(op, dt, n)
        got = O.chain_fold(dev_op, dt, arg, dev_op == O.DEV_PREMULSUM, ins)
        # the chain folds from the leaf up: x[n-1] first, x[0] last
        exp = _left_fold(dt, op, ins[::-1])
        assert_bitexact(dt, got, exp, minmax=op in (2, 3), what=f"{O.TYPE_NAMES[dt]} {O.OP_NAMES[op]} n={n}")

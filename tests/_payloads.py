"""Special-value and order-sensitive payloads for the fold-path parity tests.

hard_input(dt, op, count, rank, n_ranks, seed) is one rank's element stream in
the storage dtype (bf16 as uint16 bits, fp8 as uint8 codes), deterministic in
its arguments.  Of every PERIOD = 257 positions the first SPAN = 61 hold the
type's specials table and the other 196 finite, order-sensitive values; 257
and 61 are co-prime to every pack, wave and line size, so specials land in
heads, tails, every lane and every channel part.

The table is written as a *chain*: rank r reads the entry STRIDE = 7 places
after rank r - 1's, so the n ranks' values at one element position are n
consecutive chain entries, and the period index rotates the whole table, so a
window meets every position of the span.  The chains below are laid out so
that their windows of 2, 3 and 4 entries produce, under every op, an infinity
(fp8: the saturated max-finite code), a -0 that survives (-0 + -0, -0 * 1),
a subnormal, x + (-x), overflow by summing, and round-to-even ties of both
parities — tests/test_payloads_cpu.py checks that from the oracle alone.

Signalling NaNs: the chain of a sum / prod / avg stream carries one signalling
NaN next to the quiet one.  A min / max stream carries quiet NaNs only: the
reference's fmin / fmax on a signalling NaN is libm-dependent (IEEE 754-2008
minNum returns a quiet NaN, C's fmin may return the other operand), so no
expected value exists for it.

At most 61 of 257 outputs can come from specials and the other positions
cannot produce a NaN, so the NaN share of any expected output stays below
25 % (assert_cap lets every test assert that and the class presence).
"""
import numpy as np

from oracle import oracle as O

PERIOD, SPAN, STRIDE = 257, 61, 7
# the collective matrix of tests/test_gpu_payloads.py (and the cap test of tests/test_payloads_cpu.py)
MATRIX_TYPES = (6, 9, 7, 8, 10, 11, 0, 2, 5)  # f16 bf16 f32 f64 e4m3 e5m2 i8 i32 u64
MATRIX_OPS = (0, 1, 2, 3, 4)
MATRIX_RANKS = (2, 3, 4)
AR_COUNT, RS_COUNT, SEED = 8209, 2053, 20261
# IEEE-like layouts (exponent bits, mantissa bits) of the float types
FLOAT_FMT = {6: (5, 10), 7: (8, 23), 8: (11, 52), 9: (8, 7)}
INT_TYPES = (0, 1, 2, 3, 4, 5)
F8_TYPES = (10, 11)
_UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
# fp8 codes by name: E4M3 (bias 7, no infinity, NaN = S.1111.111) / E5M2
_F8 = {10: dict(one=0x38, one_ulp=0x39, ulp_half=0x18, maxf=0x7e, minnorm=0x08, half=0x30, maxsub=0x07,
                minsub=0x01, nan_pos=0x7f, nan_neg=0xff),
       11: dict(one=0x3c, one_ulp=0x3d, ulp_half=0x30, maxf=0x7b, minnorm=0x04, half=0x38, maxsub=0x03,
                minsub=0x01, nan_pos=0x7e, nan_neg=0xfd)}


def _storage(dt):
    return np.dtype(O.NP_DTYPE[dt])


def _float_chain(dt, op):
    e_bits, m = FLOAT_FMT[dt]
    s = 1 << (e_bits + m)
    expmask = ((1 << e_bits) - 1) << m
    bias = (1 << (e_bits - 1)) - 1

    def val(e, frac=0):  # 2^e * (1 + frac / 2^m)
        return ((e + bias) << m) | frac

    one, inf, maxf = val(0), expmask, expmask - 1
    qnan = expmask | (1 << (m - 1)) | 0x15  # quiet, with a payload
    # a signalling NaN (quiet bit clear) for sum / prod / avg; min / max: a second quiet one
    nan2 = expmask | 0x2a | (0 if op in (0, 1, 4) else 1 << (m - 1))
    top, half_max = val(bias), maxf - (1 << m)  # 2^emax (top + top overflows), max / 2 (sums to max)
    minsub, maxsub, minnorm = 1, (1 << m) - 1, 1 << m
    one_ulp, ulp_half = one | 1, val(-(m + 1))  # (1 + ulp) + ulp/2 and 1 + ulp/2: ties of both parities
    pi = val(1, 73 << (m - 7))  # 3.140625
    return ([s] * 4 + [one] * 3 +  # -0 + -0 (+ -0 + -0) = -0; -0 * 1 * 1 * 1 = -0; 1 + 1 + 1 + inf
            [inf, maxf, s | maxf, s | inf, s | one, qnan, one_ulp, ulp_half, one, nan2,
             top, top, half_max, half_max, s | half_max, s | top, pi, s | pi,
             0, 0, 0, maxsub, minnorm, val(-1), one, one,  # 0 + 0 + 0 + maxsub; minnorm * 0.5: subnormal
             minsub, s | minsub, s | maxsub, s | one_ulp, s | ulp_half])


def _f8_chain(dt):
    c = _F8[dt]
    s = 0x80
    return ([s] * 4 + [c["one"]] * 3 +
            [0x7c, c["maxf"], s | c["maxf"], 0xfc, s | c["one"], c["nan_pos"], c["one_ulp"], c["ulp_half"],
             c["one"], c["nan_neg"]] + [c["maxf"]] * 4 + [s | c["maxf"]] +  # max + max saturates
            [0, 0, 0, c["maxsub"], c["minnorm"], c["half"], c["one"], c["one"],
             c["minsub"], s | c["minsub"], s | c["maxsub"], s | c["one_ulp"], s | c["ulp_half"], 0x7c])


def _int_chain(dt):
    bits = 8 * _storage(dt).itemsize
    mask = (1 << bits) - 1
    signed = dt in (0, 2, 4)
    lo = -(1 << (bits - 1)) if signed else 0
    hi = (1 << (bits - 1)) - 1 if signed else mask
    rep = lambda b: int.from_bytes(bytes([b]) * (bits // 8), "little")  # noqa: E731
    chain = [lo, 0, 0, 0, hi, 1, -1, lo + 1]  # min + 0: a SumPostDiv dividend at the signed minimum
    for n in range(2, 9):
        chain += [hi // n + 1, hi // n - 1]
    chain += [rep(0x7f), rep(0x80), rep(0xff)]  # the SWAR carries
    return [v & mask for v in chain]


def table(dt, op=0):
    """The specials table of (dt, op) in the storage dtype: entry (STRIDE * m)
    % L is the m-th entry of the type's chain."""
    chain = _float_chain(dt, op) if dt in FLOAT_FMT else _f8_chain(dt) if dt in F8_TYPES else _int_chain(dt)
    n = len(chain)
    assert n <= SPAN and np.gcd(n, STRIDE) == 1
    st = _storage(dt)
    t = np.zeros(n, _UINT[st.itemsize])
    t[(STRIDE * np.arange(n)) % n] = np.array(chain, dtype=np.uint64).astype(t.dtype)
    return t.view(st)


def _f8_codes(dt, x):
    """RN-even f32 -> fp8 code for |x| < 2 (neither saturation nor NaN in range)."""
    vals = O.fp8_bits_to_f32(dt, np.arange(128, dtype=np.uint8))
    vals = np.where(np.isnan(vals), np.inf, vals)
    a = np.abs(x)
    hi = np.clip(np.searchsorted(vals, a), 1, 127)  # vals[hi - 1] < a <= vals[hi]
    lo = hi - 1
    dlo, dhi = a - vals[lo], vals[hi] - a
    pick = np.where((dhi < dlo) | ((dhi == dlo) & (hi % 2 == 0)), hi, lo)
    return (pick | np.where(np.signbit(x), 0x80, 0)).astype(np.uint8)


def _fill(rng, dt, op, count):
    """The finite, order-sensitive values of the other positions."""
    st = _storage(dt)
    if dt in INT_TYPES:
        if op == 1:
            return rng.integers(1, 4, count).astype(st)
        return rng.integers(0, 1 << 64, count, dtype=np.uint64).astype(_UINT[st.itemsize]).view(st)
    if dt in F8_TYPES:
        return _f8_codes(dt, rng.uniform(-2, 2, count).astype(np.float32))
    if op == 1:
        x = rng.uniform(0.5, 2.0, count) * rng.choice([-1.0, 1.0], count)
    else:
        x = rng.uniform(-1, 1, count) * 2.0 ** rng.integers(-10, 11, count)
    return O.f32_to_bf16_bits(x.astype(np.float32)) if dt == 9 else x.astype(st)


def hard_input(dt, op, count, rank, n_ranks, seed):
    """Rank `rank`'s stream of `count` elements (see the module docstring)."""
    rng = np.random.default_rng([seed, dt, op, rank, n_ranks])
    x = _fill(rng, dt, op, count)
    t = table(dt, op)
    pos = np.arange(count)
    j, k = pos % PERIOD, pos // PERIOD
    sp = j < SPAN
    x[sp] = t[(j[sp] + STRIDE * rank + k[sp]) % t.size]
    return x


def all_pairs_u8():
    """Every (a, b) byte pair: 65 536 elements each."""
    codes = np.arange(256, dtype=np.uint8)
    return np.repeat(codes, 256), np.tile(codes, 256)


def special_pairs(dt, op=0):
    """The cross product of (dt, op)'s table with itself, as two streams."""
    t = table(dt, op)
    return np.repeat(t, t.size), np.tile(t, t.size)


def classes(dt, a):
    """Element counts of a float array by class: nan, finite (non-zero), inf
    (fp8: the saturated max-finite code), negzero, subnormal."""
    a = np.ascontiguousarray(a)
    u = a.view(_UINT[a.dtype.itemsize]).astype(np.uint64)
    if dt in F8_TYPES:
        mag, s, m = u & 0x7f, 0x80, (3 if dt == 10 else 2)
        nan = mag == 0x7f if dt == 10 else mag > 0x7c
        inf = mag == _F8[dt]["maxf"]
        finite = ~nan
    else:
        e_bits, m = FLOAT_FMT[dt]
        s = 1 << (e_bits + m)
        expmask = ((1 << e_bits) - 1) << m
        mag = u & (s - 1)
        nan, inf = mag > expmask, mag == expmask
        finite = mag < expmask
    return {"nan": int(nan.sum()), "finite": int((finite & (mag > 0)).sum()), "inf": int(inf.sum()),
            "negzero": int((u == s).sum()), "subnormal": int(((mag > 0) & (mag < (1 << m))).sum())}


def assert_cap(dt, expected, what=""):
    """The payload contract on one expected output: NaNs at most 25 %, and a
    float output holds a finite non-zero, an infinite / saturated, a -0 and a
    subnormal element."""
    if dt in INT_TYPES:
        return
    c = classes(dt, expected)
    assert 4 * c["nan"] <= np.asarray(expected).size, f"{what}: NaN share {c}"
    missing = [k for k in ("finite", "inf", "negzero", "subnormal") if c[k] == 0]
    assert not missing, f"{what}: expected output lacks {missing} ({c})"

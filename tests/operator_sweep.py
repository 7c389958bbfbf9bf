"""
The cases and references of the operator sweep (tests/test_operator_sweep_host.py, tests/test_gpu_operator_sweep.py): every
template instantiation of the band kernels (band_apply / band_apply_line, band_absmax / band_absmax_line: 42 each) and of the
product kernels (band_product_line / band_product_tile: 100) on the smallest shapes that cross each constant of its launch
geometry.  NumPy and ``fractions`` only: no GPU import, and the library is not imported here either.

Every map is made by hand: ``first``, ``f``, ``g`` are shaped at will and the weights chosen.

    exact cases   weights are multiples of 2^-3 in [-1, 1] with exact zeros, data are small integers: every partial sum, in
                  any order and with or without contraction, is exact in fp64 and every output is a dtype value, so the
                  int64 evaluation below is THE result, byte for byte (``band_exact``, ``absmax_exact``, ``product_exact``)
    real cases    standard-normal data, random real weights; the exact rational value is formed from the stored doubles in
                  Python integers on a common power of two (``to_ints``: the same numbers as ``Fraction(float)``)

The launch geometry is restated here from the launchers (bsk_refine_tu.hip, bsk_product_tu.hip) and the constants from the
headers; the host test reads the headers and asserts that the constants below are the built ones.
"""
import functools
import zlib
from collections import namedtuple
from fractions import Fraction

import numpy as np

# ------------------------------------------------------------------------------------------ the kernels' constants
BAND_BLOCK, BAND_ROWS, BAND_LINE_LDS, ABSMAX_PARTS = 256, 32, 4096, 1024
PROD_BLOCK, PROD_LINE_LDS, TILE_R1, TILE_R2, TILE_LDS = 256, 2048, 16, 64, 2560
HEADER_CONSTANTS = {
    "bsk_refine.hpp": {"BAND_BLOCK": BAND_BLOCK, "BAND_ROWS": BAND_ROWS, "LINE_LDS": BAND_LINE_LDS},
    "bsk_refine_tu.hip": {"ABSMAX_PARTS": ABSMAX_PARTS},
    "bsk_product.hpp": {"PROD_BLOCK": PROD_BLOCK, "LINE_LDS": PROD_LINE_LDS, "TILE_R1": TILE_R1, "TILE_R2": TILE_R2,
                        "TILE_LDS": TILE_LDS},
}

DTYPES = (np.float32, np.float64)
BAND_KS = (2, 3, 4, 5, 6, 7, 8)
PROD_KS = (2, 3, 4, 5, 6)
LANES = ("wide", "scalar", "line")

BandInst = namedtuple("BandInst", "dtype K lanes")
ProdInst = namedtuple("ProdInst", "dtype k1 k2 kernel")

BAND_INSTANCES = [BandInst(dt, K, lanes) for dt in DTYPES for K in BAND_KS for lanes in LANES]
PRODUCT_INSTANCES = [ProdInst(dt, k1, k2, kernel) for dt in DTYPES for k1 in PROD_KS for k2 in PROD_KS for kernel in ("line", "tile")]


def tag(dtype):
    return "f32" if np.dtype(dtype) == np.float32 else "f64"


def band_id(inst):
    return f"{tag(inst.dtype)}-K{inst.K}-{inst.lanes}"


def product_id(inst):
    return f"{tag(inst.dtype)}-k{inst.k1}x{inst.k2}-{inst.kernel}"


def lane_width(dtype):
    """Elements of a 16-byte lane."""
    return 16 // np.dtype(dtype).itemsize


def rng_of(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


# ------------------------------------------------------------------------------------------ first columns
def first_pattern(kind, n_out, K, rng):
    """first[j] of one of the window patterns: "const" (the window never moves), "step1", "step2", "mix" (0 / 1 as refinement
    makes), "jumps" (mix with one jump of exactly K and one of K + 3, both inside the first row block: the window is
    replaced completely twice), "boundary" (mix with a jump of K + 3 from row 31 to row 32)."""
    step = np.zeros(n_out, np.int64)
    if kind == "step1":
        step[1:] = 1
    elif kind == "step2":
        step[1:] = 2
    elif kind in ("mix", "jumps", "boundary"):
        step[1:] = rng.integers(0, 2, n_out - 1)
        if n_out > 1:
            step[n_out // 2] = 1                      # never all zero
    if kind == "jumps":
        r1, r2 = min(n_out // 3, 9), min(2 * n_out // 3, 20)
        if 1 <= r1 < r2:
            step[r1], step[r2] = K, K + 3
    if kind == "boundary":
        assert n_out > BAND_ROWS
        step[BAND_ROWS] = K + 3
    return np.cumsum(step).astype(np.int32)


def eighths(rng, shape):
    """Integers w8 in [-8, 8], a fifth of them 0: the weights are w8 / 8."""
    w8 = rng.integers(-8, 9, shape)
    w8[rng.random(shape) < 0.2] = 0
    return w8.astype(np.int64)


def max_span(first, K, rows):
    """BandMap::max_span / ProductVar::max_span of one operand."""
    first = np.asarray(first, np.int64)
    n = len(first)
    return max(int(first[min(j0 + rows, n) - 1]) + K - int(first[j0]) for j0 in range(0, n, rows))


# ------------------------------------------------------------------------------------------ band cases
# how: "plain", "offset" (the input one element off 16-byte alignment), "minus_offset" (only the subtrahend of absmax is)
BandCase = namedtuple("BandCase", "name first w8 nIn outer inner how only_absmax")

ROWS_NOUT = (1, 31, 32, 33, 65)
ROWS_PATTERNS = ("const", "step1", "mix", "jumps", "boundary")
LINE_NOUT = (1, 3, 64, 255, 256, 257)
LINE_PATTERNS = ("mix", "const", "step1", "jumps")


def rows_geometry(inner, V):
    """launch_rows / absmax_rows: lanes along inner, LX (a power of two), LY = lines of outer per workgroup, inner tiles."""
    lanes = inner // V
    LX = 1
    while LX < BAND_BLOCK and LX < lanes:
        LX *= 2
    return LX, BAND_BLOCK // LX, (lanes + LX - 1) // LX


def line_geometry(first, K, nlines):
    """launch_line / absmax_line: R rows per tile, G line groups, staged, NL before the cut to the line count."""
    R = min(len(first), BAND_BLOCK)
    G = BAND_BLOCK // R
    span = max_span(first, K, R)
    staged = span <= BAND_LINE_LDS
    NL0 = min(BAND_LINE_LDS // span, 16 * G) if staged else G
    return R, G, staged, NL0, max(1, min(NL0, nlines))


def _band_case(name, first, K, outer, inner, how="plain", only_absmax=False):
    first = np.asarray(first, np.int32)
    return BandCase(name, first, eighths(rng_of("w", name, K), (len(first), K)), int(first[-1]) + K, outer, inner, how, only_absmax)


@functools.lru_cache(maxsize=None)
def band_cases(K, lanes, V):
    """The edge cases of one instantiation (the dtype enters through V = elements of a 16-byte lane only).

    wide / scalar (band_apply, band_absmax): nOut 1, 31, 32, 33, 65 x lanes along inner (wide: inner / V = 1, 3, 257, so LX = 1,
    4, 256 and a second inner tile of one lane; scalar: odd inner 3 and 257, and the wide-eligible inner V and 3 V behind a
    misaligned pointer - inner == 1 is the line kernel, so scalar lanes never run LX = 1); outer 1, LY - 1, LY + 1 in turn, so
    that every inner meets each; the five window patterns in turn, so that every inner meets each.  One more shape, for
    absmax alone, has more units than ABSMAX_PARTS (1025 units of one workgroup each: two units per workgroup, the last one).
    line (band_apply_line, band_absmax_line): nOut 1, 3, 64, 255, 256, 257 (R = 3 leaves one lane idle, G = 85, 4, 1, and a
    second tile of one row) x nlines 1, NL - 1, NL, NL + 1, and two two-row maps whose max_span is LINE_LDS (staged, NL = 1) and
    LINE_LDS + 1 (read in place); one more, for absmax alone, with 1025 line blocks."""
    cases = []
    if lanes == "line":
        for i_n, n_out in enumerate(LINE_NOUT):
            kind = LINE_PATTERNS[i_n % len(LINE_PATTERNS)]
            first = first_pattern(kind, n_out, K, rng_of("line", n_out, K))
            NL0 = line_geometry(first, K, 1 << 30)[3]
            for nlines in sorted({1, NL0 - 1, NL0, NL0 + 1} - {0}):
                cases.append(_band_case(f"line-n{n_out}-{kind}-l{nlines}", first, K, nlines, 1))
        cases.append(_band_case("line-lds-exact", [0, BAND_LINE_LDS - K], K, 3, 1))
        cases.append(_band_case("line-lds-plus-one", [0, BAND_LINE_LDS - K + 1], K, BAND_BLOCK // 2 + 1, 1))
        cases.append(_band_case("line-many-blocks", [0, BAND_LINE_LDS // 2 + 1 - K], K, ABSMAX_PARTS + 1, 1, only_absmax=True))
        return tuple(cases)
    if lanes == "wide":
        inners = [(V, "plain"), (3 * V, "plain"), (257 * V, "plain")]
    else:
        inners = [(3, "plain"), (257, "plain"), (V, "offset"), (3 * V, "minus_offset")]
    for i_n, n_out in enumerate(ROWS_NOUT):
        for i_i, (inner, how) in enumerate(inners):
            LY = rows_geometry(inner, V if lanes == "wide" else 1)[1]
            outers = sorted({1, LY - 1, LY + 1} - {0})
            outer = outers[i_n % len(outers)]
            kind = ROWS_PATTERNS[(i_n + i_i) % len(ROWS_PATTERNS)]
            if kind == "boundary" and n_out <= BAND_ROWS:
                kind = "jumps"
            first = first_pattern(kind, n_out, K, rng_of("rows", n_out, inner, K))
            cases.append(_band_case(f"rows-n{n_out}-{kind}-o{outer}-i{inner}-{how}", first, K, outer, inner, how))
    inner = 255 * V if lanes == "wide" else 255
    cases.append(_band_case(f"rows-many-units-i{inner}", [0, 0], K, ABSMAX_PARTS + 1, inner, only_absmax=True))
    return tuple(cases)


def band_weights(case):
    return case.w8.astype(np.float64) / 8.0


def band_int_data(case, dtype):
    """(data, minus) of an exact case: integers in [-64, 64] and [-512, 512]."""
    rng = rng_of("data", case.name, len(case.first))
    x = rng.integers(-64, 65, (case.outer, case.nIn, case.inner))
    minus = rng.integers(-512, 513, (case.outer, len(case.first), case.inner))
    return x.astype(dtype), minus.astype(dtype)


def band_real_case(case, dtype):
    """(w, data, minus) of the real-valued twin of a case: random real weights, standard-normal data."""
    rng = rng_of("real", case.name, len(case.first))
    w = rng.uniform(-1.0, 1.0, case.w8.shape)
    x = rng.standard_normal((case.outer, case.nIn, case.inner)).astype(dtype)
    minus = rng.standard_normal((case.outer, len(case.first), case.inner)).astype(dtype)
    return w, x, minus


def band_eval(first, w, x):
    """out[o, j, i] = sum_t w[j, t] x[o, first[j] + t, i] in the arithmetic of the arrays' dtype (int64, object, float64)."""
    first = np.asarray(first, np.int64)
    out = None
    for t in range(w.shape[1]):
        term = w[:, t][None, :, None] * x[:, first + t, :]
        out = term if out is None else out + term
    return out


def band_exact8(case, x):
    """8 x the exact result of an exact case, int64."""
    return band_eval(case.first, case.w8, x.astype(np.int64))


def band_exact(case, x):
    """The exact result as the data's type (the host test asserts that it is representable)."""
    return (band_exact8(case, x).astype(np.float64) / 8.0).astype(x.dtype)


def absmax_exact(case, x, groups, minus=None):
    """(groups, nOut) float64: max over the lines of a group of |exact row - minus|."""
    r8 = band_exact8(case, x)
    if minus is not None:
        r8 = r8 - 8 * minus.astype(np.int64)
    n_out = len(case.first)
    m8 = np.abs(r8).reshape(groups, case.outer // groups, n_out, case.inner).max(axis=(1, 3))
    return m8.astype(np.float64) / 8.0


# ------------------------------------------------------------------------------------------ product cases
# variables: [(f, g, W8 (nOut, k1, k2) int64, nIn1, nIn2)]; terms (P, T, 3); limit: the data are integers in [-limit, limit]
ProdCase = namedtuple("ProdCase", "name variables PA PB terms limit")

PROD_LINE_PAIRS = (("mix", "step2"), ("step1", "const"), ("const", "mix"), ("step2", "mix"), ("jumps", "step1"), ("mix", "const"))
TERM_COUNTS = (1, 3, 2)


def product_line_geometry(f, g, k1, k2, T, P):
    """launch_line of bsk_product_tu.hip: R, G, staged, NP before the cut to the plane count, NP."""
    R = min(len(f), PROD_BLOCK)
    G = PROD_BLOCK // R
    per_plane = T * max(max_span(f, k1, R), max_span(g, k2, R))
    staged = per_plane <= PROD_LINE_LDS
    NP0 = min(PROD_LINE_LDS // per_plane, 16 * G) if staged else G
    return R, G, staged, NP0, max(1, min(NP0, P))


def tile_staged(variables):
    """launch_tile's decision: both operands' pieces under a 16 x 64 tile fit TILE_LDS."""
    (f1, g1, W1, _, _), (f2, g2, W2, _, _) = variables
    ua, ub = max_span(f1, W1.shape[1], TILE_R1), max_span(g1, W1.shape[2], TILE_R1)
    va, vb = max_span(f2, W2.shape[1], TILE_R2), max_span(g2, W2.shape[2], TILE_R2)
    return ua * va <= TILE_LDS and ub * vb <= TILE_LDS, (ua * va, ub * vb)


def plane_terms(rng, P, T, PA, PB):
    """A plane table by hand: any planes of a and b; T = 2 is signed as a cross product is (+, -)."""
    terms = np.empty((P, T, 3), np.int32)
    terms[:, :, 0] = rng.integers(0, PA, (P, T))
    terms[:, :, 1] = rng.integers(0, PB, (P, T))
    terms[:, :, 2] = 1
    if T == 2:
        terms[:, 1, 2] = -1
    return terms


def _variable(name, f, g, k1, k2):
    f, g = np.asarray(f, np.int32), np.asarray(g, np.int32)
    return (f, g, eighths(rng_of("W", name, k1, k2), (len(f), k1, k2)), int(f[-1]) + k1, int(g[-1]) + k2)


def _product_case(name, variables, P, T, limit):
    PA, PB = 3, 2
    return ProdCase(name, variables, PA, PB, plane_terms(rng_of("terms", name, P, T), P, T, PA, PB), limit)


@functools.lru_cache(maxsize=None)
def product_cases(k1, k2, kernel):
    """The edge cases of one instantiation.

    line: nOut 1, 3, 64, 255, 256, 257 x P 1, NP, NP + 1, T = 1 (scalar), 3 (dot), 2 signed (cross) in turn; f and g move
    differently (one operand's piece is much longer than the other's); two-row maps with T max(sa, sb) = 2048 through a
    (T = 2) and through b (T = 1): staged, NP = 1; and 2049 through a (T = 3) and through b (T = 1): read in place.
    tile: (N1, N2) = (1, 1), (15, 63), (16, 64), (17, 65) with variable 1 at the orders (k2, k1), (17, 65) once more with
    variable 1 at (2, 6); T in turn; maps with ua va = 2560 (staged), 2561 (in place), and ub vb = 2561 with a small a."""
    cases = []
    if kernel == "line":
        for i_n, n_out in enumerate(LINE_NOUT):
            kf, kg = PROD_LINE_PAIRS[i_n]
            T = TERM_COUNTS[i_n % 3]
            f = first_pattern(kf, n_out, k1, rng_of("f", n_out, k1, k2))
            g = first_pattern(kg, n_out, k2, rng_of("g", n_out, k1, k2))
            NP0 = product_line_geometry(f, g, k1, k2, T, 1 << 30)[3]
            for P in sorted({1, NP0, NP0 + 1}):
                name = f"line-n{n_out}-{kf}-{kg}-T{T}-P{P}"
                cases.append(_product_case(name, (_variable(name, f, g, k1, k2),), P, T, 64))
        half, third = PROD_LINE_LDS // 2, (PROD_LINE_LDS + 1) // 3
        assert 2 * half == PROD_LINE_LDS and 3 * third == PROD_LINE_LDS + 1
        for name, f, g, T, P in (("line-lds-exact-a", [0, half - k1], [0, 1], 2, 3),
                                 ("line-lds-exact-b", [0, 1], [0, PROD_LINE_LDS - k2], 1, 3),
                                 ("line-lds-plus-one-a", [0, third - k1], [0, 0], 3, PROD_BLOCK // 2 + 2),
                                 ("line-lds-plus-one-b", [0, 1], [0, PROD_LINE_LDS + 1 - k2], 1, 3)):
            cases.append(_product_case(name, (_variable(name, f, g, k1, k2),), P, T, 64))
        return tuple(cases)
    shapes = [(1, 1, (k2, k1)), (15, 63, (k2, k1)), (16, 64, (k2, k1)), (17, 65, (k2, k1)), (17, 65, (2, 6))]
    kinds = [("mix", "const", "mix", "step2"), ("step1", "mix", "const", "mix")]
    for i_s, (N1, N2, (k1u, k2u)) in enumerate(shapes):
        T = TERM_COUNTS[i_s % 3]
        a1, b1, a2, b2 = kinds[i_s % 2]
        name = f"tile-{N1}x{N2}-u{k1u}x{k2u}-T{T}"
        u = _variable(name + "-u", first_pattern(a1, N1, k1u, rng_of("f1", name)), first_pattern(b1, N1, k2u, rng_of("g1", name)), k1u, k2u)
        v = _variable(name + "-v", first_pattern(a2, N2, k1, rng_of("f2", name)), first_pattern(b2, N2, k2, rng_of("g2", name)), k1, k2)
        cases.append(_product_case(name, (u, v), 2, T, 3))
    k1u, k2u = k2, k1
    for name, f1, g1, f2, g2, T in (("tile-lds-exact-a", [0, 40 - k1u], [0, 1], [0, 64 - k1], [0, 1], 2),
                                    ("tile-lds-plus-one-a", [0, 13 - k1u], [0, 0], [0, 197 - k1], [0, 1], 3),
                                    ("tile-lds-plus-one-b", [0, 1], [0, 13 - k2u], [0, 0], [0, 197 - k2], 1)):
        cases.append(_product_case(name, (_variable(name + "-u", f1, g1, k1u, k2u), _variable(name + "-v", f2, g2, k1, k2)), 2, T, 3))
    return tuple(cases)


def product_weights(case):
    """The variables as ``product.ProductMap`` takes them."""
    return [(f, g, W8.astype(np.float64) / 8.0, n1, n2) for f, g, W8, n1, n2 in case.variables]


def product_int_data(case, dtype):
    rng = rng_of("data", case.name)
    a = rng.integers(-case.limit, case.limit + 1, (case.PA, *[v[3] for v in case.variables]))
    b = rng.integers(-case.limit, case.limit + 1, (case.PB, *[v[4] for v in case.variables]))
    return a.astype(dtype), b.astype(dtype)


def product_eval(variables, a, b, terms, signed=True):
    """out[p, ...] = sum_t sign sum W1 W2 A B in the arithmetic of the arrays' dtype (int64, object, float64); variables:
    [(f, g, W)] with W of that dtype.  signed=False: every sign counts as +1 (for sums of absolute values)."""
    out = None
    for t in range(terms.shape[1]):
        A, B = a[terms[:, t, 0]], b[terms[:, t, 1]]
        f2, g2, W2 = (np.asarray(variables[-1][0], np.int64), np.asarray(variables[-1][1], np.int64), variables[-1][2])

        def last(rowsA, rowsB):
            """rows (..., n), (..., m) -> (..., N): the last variable's sum."""
            acc = None
            for i in range(W2.shape[1]):
                x = rowsA[..., f2 + i]
                for l in range(W2.shape[2]):
                    term = W2[:, i, l] * x * rowsB[..., g2 + l]
                    acc = term if acc is None else acc + term
            return acc

        if len(variables) == 1:
            acc = last(A, B)
        else:
            f1, g1, W1 = np.asarray(variables[0][0], np.int64), np.asarray(variables[0][1], np.int64), variables[0][2]
            acc = None
            for i in range(W1.shape[1]):
                for l in range(W1.shape[2]):
                    term = W1[:, i, l][None, :, None] * last(A[:, f1 + i, :], B[:, g1 + l, :])
                    acc = term if acc is None else acc + term
        if signed:
            sign = terms[:, t, 2].astype(np.int64).reshape((-1,) + (1,) * (acc.ndim - 1))
            acc = acc * sign if acc.dtype != object else acc * sign.astype(object)
        out = acc if out is None else out + acc
    return out


def product_denominator(case):
    return 8 ** len(case.variables)


def product_exact_scaled(case, a, b):
    """(exact result, sum of the absolute values of its elementary products), both times 8^M, int64."""
    ints = [(f, g, W8) for f, g, W8, _, _ in case.variables]
    A, B = a.astype(np.int64), b.astype(np.int64)
    absolute = [(f, g, np.abs(W8)) for f, g, W8 in ints]
    return product_eval(ints, A, B, case.terms), product_eval(absolute, np.abs(A), np.abs(B), case.terms, signed=False)


def product_exact(case, a, b):
    return (product_exact_scaled(case, a, b)[0].astype(np.float64) / product_denominator(case)).astype(a.dtype)


# ------------------------------------------------------------------------------------------ exact rationals of doubles
def to_ints(x):
    """(n, e): object array of Python integers and an exponent with x == n * 2^e exactly, for finite float arrays."""
    x = np.asarray(x, np.float64)
    m, e = np.frexp(x)
    mant = (m * 2.0 ** 53).astype(np.int64)                     # exact: |m| < 1 has 53 bits
    nz = x != 0
    emin = int(e[nz].min()) if nz.any() else 0
    shift = np.where(nz, e - emin, 0).astype(np.int64)
    n = mant.astype(object) * np.array([1 << int(s) for s in shift.reshape(-1)], object).reshape(x.shape)
    return n, emin - 53


def fractions_of(n, e):
    """The object array n * 2^e as Fractions (flat list)."""
    scale = Fraction(2) ** e
    return [Fraction(int(v)) * scale for v in n.reshape(-1)]


def band_real_exact(first, w, x):
    """The exact rational rows of a real-valued band case (flat list of Fractions) and sum_t |w x| as float64."""
    wn, we = to_ints(w)
    xn, xe = to_ints(x)
    exact = fractions_of(band_eval(first, wn, xn), we + xe)
    return exact, band_eval(first, np.abs(w), np.abs(np.asarray(x, np.float64))).reshape(-1)


def product_real_case(inst):
    """The real-valued case of (d): the (17, 65) tile shape with variable 1 at (k2, k1), or the 257-row line; T = 2 signed;
    standard-normal data, random real weights.  Returns (variables as ProductMap takes them, a, b, terms, n of the bar)."""
    k1, k2 = inst.k1, inst.k2
    rng = rng_of("product real", k1, k2, inst.kernel)
    T = 2

    def variable(N, ka, kb, kf, kg):
        f, g = first_pattern(kf, N, ka, rng), first_pattern(kg, N, kb, rng)
        return (f, g, rng.uniform(-1.0, 1.0, (N, ka, kb)), int(f[-1]) + ka, int(g[-1]) + kb)

    if inst.kernel == "line":
        variables = [variable(257, k1, k2, "mix", "step2")]
        P, n = 3, k1 + k2 + T + 1
    else:
        variables = [variable(17, k2, k1, "mix", "step1"), variable(65, k1, k2, "mix", "const")]
        P, n = 2, k1 + k2 + k2 * k1 + T + 2
    PA, PB = 3, 2
    a = rng.standard_normal((PA, *[v[3] for v in variables])).astype(inst.dtype)
    b = rng.standard_normal((PB, *[v[4] for v in variables])).astype(inst.dtype)
    return variables, a, b, plane_terms(rng, P, T, PA, PB), n


def product_real_exact(variables, a, b, terms):
    """The exact rational value of sum_terms sign sum W1 W2 A B from the stored doubles (flat list of Fractions), and the sum
    of the absolute values of the elementary products as float64 (its own relative error, below 2^-40, does not matter to a
    bar that is n 2^-52 of it)."""
    e = 0
    ints = []
    for f, g, W, _, _ in variables:
        Wn, We = to_ints(W)
        ints.append((f, g, Wn))
        e += We
    an, ae = to_ints(a)
    bn, be = to_ints(b)
    exact = fractions_of(product_eval(ints, an, bn, terms), e + ae + be)
    absolute = [(f, g, np.abs(W)) for f, g, W, _, _ in variables]
    S = product_eval(absolute, np.abs(a.astype(np.float64)), np.abs(b.astype(np.float64)), terms, signed=False)
    return exact, S.reshape(-1)


def worst_ratio(got, exact, bars):
    """max over the elements of |got - exact| / bar; got: float array, exact: flat list of Fractions, bars: flat floats."""
    worst = 0.0
    for v, x, bar in zip(np.asarray(got, np.float64).reshape(-1).tolist(), exact, bars.tolist()):
        err = abs(Fraction(v) - x)
        if err:
            worst = max(worst, float(err / Fraction(bar)) if bar > 0.0 else np.inf)
    return worst


def counted_bars(n, unit, S, exact, dtype):
    """n * unit * S per element, plus 2^-24 |exact| for float32 (the one rounding to the data's type)."""
    bars = n * unit * np.asarray(S, np.float64)
    if np.dtype(dtype) == np.float32:
        bars = bars + 2.0 ** -24 * np.array([abs(float(x)) for x in exact])
    return bars


def bits(a):
    return np.ascontiguousarray(a).tobytes()

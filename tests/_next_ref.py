"""Plain numpy restatements of the operations beside the hot path (csrc/next.hip, gemm.hip, activation.hip), for the
kernel-level tests test_next_ops.py, test_gemm_splitk.py and test_activation_maps.py. TEST INFRASTRUCTURE ONLY.

Each function states what the REFERENCE computes (bcnn_eltwise_layer.c:111-161, bcnn_mat.c:159-177, bcnn_fc_layer.c:156-175,
bcnn_softmax_layer.c:88-155, bcnn_activation_layer.c:90-226), in float32 with the reference's order of operations where
the comparison is bit-exact and in float64 where the bar is a tolerance. test_next_ref_pinning.py runs the reference
itself on the CPU against these forms, so they are a statement of the reference and not of the HIP code.

The module also holds the guarded device buffers the kernel tests share: every tensor a kernel touches is a view into a
larger allocation with a band of sentinel words on both sides, compared bit for bit after the call."""
import numpy as np

F32, F64 = np.float32, np.float64

(ACT_NONE, ACT_TANH, ACT_RELU, ACT_RAMP, ACT_SOFTPLUS, ACT_LRELU, ACT_ABS, ACT_CLAMP, ACT_PRELU,
 ACT_LOGISTIC) = range(10)
ACT_NAMES = {ACT_NONE: "none", ACT_TANH: "tanh", ACT_RELU: "relu", ACT_RAMP: "ramp", ACT_SOFTPLUS: "softplus",
             ACT_LRELU: "lrelu", ACT_ABS: "abs", ACT_CLAMP: "clamp", ACT_PRELU: "prelu", ACT_LOGISTIC: "logistic"}

# how a result is compared (ISSUE section 1, "bars, derived rather than measured")
EXACT, FMA, ACT = "exact", "fma", "act"
FMA_TOL = 2.0 ** -23   # |got - want| <= FMA_TOL * max(1, |want|): one multiply-add the compiler may contract
# every step is one correctly rounded fp32 operation: bit-exact
FWD_BAR = {ACT_NONE: EXACT, ACT_RELU: EXACT, ACT_LRELU: EXACT, ACT_ABS: EXACT, ACT_CLAMP: EXACT, ACT_PRELU: EXACT,
           ACT_RAMP: FMA,                                     # x * (x > 0) + 0.1f * x
           ACT_TANH: ACT, ACT_SOFTPLUS: ACT, ACT_LOGISTIC: ACT}   # exp / log in double, then rounded
BWD_BAR = {ACT_NONE: EXACT, ACT_RELU: EXACT, ACT_LRELU: EXACT, ACT_ABS: EXACT, ACT_CLAMP: EXACT, ACT_PRELU: EXACT,
           ACT_RAMP: EXACT,                                   # (y > 0) + 0.1f is an add feeding a multiply
           ACT_LOGISTIC: EXACT,                               # (1 - y) * y: a subtract feeding a multiply
           ACT_TANH: FMA,                                     # 1 - y * y
           ACT_SOFTPLUS: ACT}


# ---- the activation map ---------------------------------------------------------------------------------------------------
def act_forward32(x, act, slope=None):
    """bcnn_forward_activation_cpu on float32 values, every operation rounded to float32 on its own (exp / log in
    double exactly where the reference evaluates them in double). `slope` broadcasts against x (PReLU)."""
    x = np.asarray(x, F32)
    pos = (x > 0).astype(F32)
    if act == ACT_TANH:
        e = np.exp((F32(2) * x).astype(F64))
        return ((e - 1).astype(F32) / (e.astype(F32) + F32(1))).astype(F32)
    if act == ACT_RELU:
        return x * pos                                   # a multiply: -0.0 for negatives
    if act == ACT_LRELU:
        return np.where(x > 0, x, F32(0.1) * x).astype(F32)
    if act == ACT_RAMP:
        return (x * pos + F32(0.1) * x).astype(F32)
    if act == ACT_SOFTPLUS:
        return np.log((F32(1) + np.exp(x.astype(F64)).astype(F32)).astype(F64)).astype(F32)
    if act == ACT_ABS:
        return np.abs(x)
    if act == ACT_CLAMP:
        return np.where(x < 0, F32(0), np.where(x > 1, F32(1), x)).astype(F32)
    if act == ACT_LOGISTIC:
        return (F32(1) / (F32(1) + np.exp(-x.astype(F64)).astype(F32))).astype(F32)
    if act == ACT_PRELU:
        return np.where(x > 0, x, np.asarray(slope, F32) * x).astype(F32)
    return x.copy()


def act_forward64(x, act, slope=None):
    """the same map evaluated in float64 on the float32 argument (the reference the exp / log activations are held to)"""
    x = np.asarray(x, F32).astype(F64)
    if act == ACT_TANH:
        return np.tanh(x)
    if act == ACT_RELU:
        return x * (x > 0)
    if act == ACT_LRELU:
        return np.where(x > 0, x, F64(F32(0.1)) * x)
    if act == ACT_RAMP:
        return x * (x > 0) + F64(F32(0.1)) * x
    if act == ACT_SOFTPLUS:
        return np.log1p(np.exp(x))
    if act == ACT_ABS:
        return np.abs(x)
    if act == ACT_CLAMP:
        return np.clip(x, 0.0, 1.0)
    if act == ACT_LOGISTIC:
        return 1.0 / (1.0 + np.exp(-x))
    if act == ACT_PRELU:
        return np.where(x > 0, x, np.asarray(slope, F32).astype(F64) * x)
    return x


def act_factor32(y, act, slope=None):
    """the derivative factor from the POST-activation value, bcnn_backward_activation_cpu, in float32 operations"""
    y = np.asarray(y, F32)
    one = F32(1)
    if act == ACT_TANH:
        return (one - y * y).astype(F32)
    if act == ACT_RELU:
        return (y > 0).astype(F32)
    if act == ACT_LRELU:
        return np.where(y > 0, one, F32(0.1)).astype(F32)
    if act == ACT_RAMP:
        return ((y > 0).astype(F32) + F32(0.1)).astype(F32)
    if act == ACT_SOFTPLUS:
        return (one / (one + np.exp(-y.astype(F64)).astype(F32))).astype(F32)
    if act == ACT_ABS:
        return np.where(y >= 0, one, -one).astype(F32)
    if act == ACT_CLAMP:
        return ((y > 0) & (y < 1)).astype(F32)
    if act == ACT_LOGISTIC:
        return ((one - y) * y).astype(F32)
    if act == ACT_PRELU:
        return np.where(y > 0, one, np.asarray(slope, F32)).astype(F32) + np.zeros_like(y)
    return np.ones_like(y)


def act_factor64(y, act):
    y = np.asarray(y, F32).astype(F64)
    if act == ACT_TANH:
        return 1.0 - y * y
    if act == ACT_SOFTPLUS:
        return 1.0 / (1.0 + np.exp(-y))
    return act_factor32(y.astype(F32), act).astype(F64)


def chan_index(n, c, hw):
    """channel of every element of a dense (n, c, hw) tensor: (i / hw) % c"""
    return (np.arange(n * c * hw, dtype=np.int64) // hw) % c


def prelu_dslopes64(x, dx, n, c, hw):
    """sum over (n, hw) of dx * x * (x < 0) per channel, in float64 (the reference accumulates it in float, in index order)"""
    x = np.asarray(x, F32).reshape(n, c, hw).astype(F64)
    dx = np.asarray(dx, F32).reshape(n, c, hw).astype(F64)
    return (dx * x * (x < 0)).sum(axis=(0, 2))


# ---- eltwise node, same-shape path ------------------------------------------------------------------------------------------
def eltwise_sum32(a, b, b_count):
    """a + (i < b_count ? b : 0), one float32 add (the reference: copy, then axpy with a = 1 over b_count elements)"""
    s = np.asarray(a, F32).copy()
    if b_count:
        s[:b_count] = s[:b_count] + np.asarray(b, F32)[:b_count]
    return s


def eltwise_forward(a, b, b_count, act):
    """(y in float32 with the reference's operation order, y in float64 from the float32 sum)"""
    s = eltwise_sum32(a, b, b_count)
    return act_forward32(s, act), act_forward64(s, act)


def eltwise_backward(y, dy, da, db, b_count, act, overwrite_a):
    """g = dy * act'(y) (dy itself for NONE); da = (overwrite_a ? 0 : da) + g; db[i] += g[i], i < b_count.
    Returns float32 (g, da, db) in the reference's operation order and the float64 g; da / db may be None."""
    dy = np.asarray(dy, F32)
    if act == ACT_NONE:
        g, g64 = dy.copy(), dy.astype(F64)
    else:
        g = (dy * act_factor32(y, act)).astype(F32)
        g64 = dy.astype(F64) * act_factor64(y, act)
    da_out = db_out = None
    if da is not None:
        base = np.zeros_like(g) if overwrite_a else np.asarray(da, F32)
        da_out = (base + g).astype(F32)
    if db is not None:
        db_out = (np.asarray(db, F32)[:b_count] + g[:b_count]).astype(F32)
    return g, da_out, db_out, g64


# ---- bcnn_axpy_strided, bcnn_mat.c:159-177 --------------------------------------------------------------------------------
def axpy_strided(nb, a, x, y, sy, sx, xdim, ydim, mindim):
    """y[n][k][j*sy][i*sy] += a * x[n][k][j*sx][i*sx] over min_c, min_h, min_w; x is (nb, xc, xh, xw), y likewise.
    Returns (float32 result with the product and the sum rounded separately, float64 result)."""
    xc, xh, xw = xdim
    yc, yh, yw = ydim
    mc, mh, mw = mindim
    x = np.asarray(x, F32).reshape(nb, xc, xh, xw)
    y32 = np.asarray(y, F32).reshape(nb, yc, yh, yw).copy()
    y64 = y32.astype(F64)
    xs = x[:, :mc, 0:(mh - 1) * sx + 1:sx, 0:(mw - 1) * sx + 1:sx]
    dst = (slice(None), slice(0, mc), slice(0, (mh - 1) * sy + 1, sy), slice(0, (mw - 1) * sy + 1, sy))
    y32[dst] = (y32[dst] + (F32(a) * xs).astype(F32)).astype(F32)
    y64[dst] = y64[dst] + F64(F32(a)) * xs.astype(F64)
    return y32, y64


def add_rowvec(y, v):
    return (np.asarray(y, F32) + np.asarray(v, F32)[None, :]).astype(F32)


# ---- softmax, bcnn_softmax_layer.c:88-155 ---------------------------------------------------------------------------------
def softmax64(x):
    """x: (n, C, HW) float32; softmax over C in float64"""
    x = np.asarray(x, F32).astype(F64)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def softmax_ref_order(x):
    """the reference's own order: float max, float sequential sum of (float)exp(x - vmax) over c, float
    lse = vmax + (float)log(sum), y = (float)exp(x - lse) with x - lse a float subtraction. Returns (y, lse)."""
    x = np.asarray(x, F32)
    vmax = x.max(axis=1)                                  # (n, HW)
    s = np.zeros_like(vmax)
    for c in range(x.shape[1]):                           # sequential over channels, vectorised over rows
        s = (s + np.exp((x[:, c, :] - vmax).astype(F64)).astype(F32)).astype(F32)
    lse = np.where(s != 0, vmax + np.log(s.astype(F64)).astype(F32), vmax - F32(100)).astype(F32)
    y = np.exp((x - lse[:, None, :]).astype(F64)).astype(F32)
    return y, lse


def softmax_bound(x):
    """Per-element RELATIVE bound of the float log-sum-exp form against float64 (ISSUE section 4):
        2 * (spacing32(|lse|) + 0.5 * spacing32(|x - lse|) + (C + 1) * 2^-23)
    y = exp(x - lse), so an absolute error of the exponent is a relative error of y: lse is rounded to float twice
    (log, then the add to vmax), x - lse once, and the C-term sum and the final conversion once per term."""
    x = np.asarray(x, F32)
    C = x.shape[1]
    x64 = x.astype(F64)
    m = x64.max(axis=1, keepdims=True)
    lse = (m + np.log(np.exp(x64 - m).sum(axis=1, keepdims=True))).astype(F32)   # (n, 1, HW)
    d = np.abs(x - lse).astype(F32)
    return 2.0 * (np.spacing(np.abs(lse)).astype(F64) + 0.5 * np.spacing(d).astype(F64) + (C + 1) * 2.0 ** -23)


def softmax_inputs(n, C, HW, seed):
    """(n, C, HW) logits, uniform in [-4, 4], with the rows (one row = one (image, position)) cycling through the edge
    patterns of ISSUE section 4; finite values only (the reference's sum == 0 branch needs exp to underflow for EVERY
    channel, the maximum included, where exp(0) = 1: it cannot be reached with finite inputs)."""
    rs = np.random.RandomState(seed)
    x = rs.uniform(-4, 4, (n, C, HW)).astype(F32)
    kinds = ["uniform", "equal", "spike60", "plus1e4", "minus1e4", "max_last", "max_at_64"]
    for r in range(n * HW):
        b, i = divmod(r, HW)
        kind = kinds[r % len(kinds)]
        if kind == "equal":
            x[b, :, i] = F32(0.7310585)
        elif kind == "spike60":
            x[b, rs.randint(C), i] += F32(60)
        elif kind == "plus1e4":
            x[b, :, i] += F32(1e4)
        elif kind == "minus1e4":
            x[b, :, i] -= F32(1e4)
        elif kind == "max_last":
            x[b, C - 1, i] = F32(5)
        elif kind == "max_at_64" and C > 64:
            x[b, 64, i] = F32(5)                          # lane 0's second element in a 64-lane sweep over C
    return x


def check_softmax(got, x, tag=""):
    """both assertions of ISSUE section 4; returns the worst (error / bound) ratio"""
    want, bound = softmax64(x), softmax_bound(x)
    got = np.asarray(got, F32).reshape(x.shape)
    assert np.all(np.isfinite(got)), tag
    ratio = np.abs(got.astype(F64) - want) / (bound * want)
    worst = float(ratio.max())
    assert worst <= 1.0, "%s: element %s off by %.3g x its bound" % (tag, np.unravel_index(ratio.argmax(), x.shape), worst)
    rows = np.abs(got.astype(F64).sum(axis=1) - 1.0)
    lim = x.shape[1] * bound.max(axis=1)
    over = rows / lim
    assert over.max() <= 1.0, "%s: row %d sums to 1 +- %.3g (limit %.3g)" % (tag, over.argmax(), rows.ravel()[over.argmax()],
                                                                         lim.ravel()[over.argmax()])
    return worst


# ---- gemm, bcnn_mat.c:2627-2650 ---------------------------------------------------------------------------------------------
def gemm_operands(ta, tb, m, n, k, lda, ldb, ldc, seed):
    """A, B as stored (row-major with leading dimensions lda / ldb; the padding columns hold values too) and C0, finite
    garbage of mixed magnitude"""
    rs = np.random.RandomState(seed)
    A = rs.uniform(-1, 1, ((k if ta else m), lda)).astype(F32)
    B = rs.uniform(-1, 1, ((n if tb else k), ldb)).astype(F32)
    C0 = (rs.uniform(-3, 3, (m, ldc)) * 10.0 ** rs.randint(-2, 3, (m, ldc))).astype(F32)
    return A, B, C0


def gemm_ops(ta, tb, m, n, k, A, B):
    opA = (A[:k, :m].T if ta else A[:m, :k]).astype(F64)
    opB = (B[:n, :k].T if tb else B[:k, :n]).astype(F64)
    return opA, opB


def gemm64(ta, tb, m, n, k, alpha, A, B, beta, C0):
    """(want, bound) over the m x n window: float64 alpha op(A) op(B) + beta C0 and the element-wise forward-error
    bound 2 (k + 2) 2^-24 (|alpha| |op(A)| |op(B)| + |beta C0|), which holds for any order of the k additions"""
    opA, opB = gemm_ops(ta, tb, m, n, k, A, B)
    c0 = C0[:, :n].astype(F64)
    al, be = F64(F32(alpha)), F64(F32(beta))
    want = al * (opA @ opB) + (be * c0 if beta != 0 else 0.0)
    bound = 2.0 * (k + 2) * 2.0 ** -24 * (abs(al) * (np.abs(opA) @ np.abs(opB)) + (np.abs(be * c0) if beta != 0 else 0.0))
    return want, bound


# ---- comparisons ----------------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(np.asarray(a, F32)).view(np.uint32)


def assert_bits(tag, got, want):
    g, w = bits(got).ravel(), bits(want).ravel()
    assert g.shape == w.shape, (tag, g.shape, w.shape)
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, ("%s: %d of %d elements differ in bits, first at %d: got %r want %r"
                           % (tag, bad.size, g.size, bad[0], np.asarray(got, F32).ravel()[bad[0]],
                              np.asarray(want, F32).ravel()[bad[0]]))


def assert_fma(tag, got, want):
    got, want = np.asarray(got, F64).ravel(), np.asarray(want, F64).ravel()
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    ratio = np.abs(got - want) / (FMA_TOL * np.maximum(1.0, np.abs(want)))
    assert np.all(np.isfinite(got)) and ratio.max(initial=0.0) <= 1.0, (
        "%s: element %d is %.9g, want %.9g (%.2f x 2^-23 max(1, |want|))"
        % (tag, ratio.argmax(), got[ratio.argmax()], want[ratio.argmax()], ratio.max()))


def assert_bar(bar, tag, got, want32, want64, act_tol):
    """EXACT: bits of the float32 restatement; FMA: 2^-23 max(1, |want|) of it; ACT: the project's activation bar
    (_golden.assert_close with act_tol, as test_hip_parity.py applies ACT_TOL) against the float64 evaluation"""
    from tests import _golden as G
    if bar == EXACT:
        assert_bits(tag, got, want32)
    elif bar == FMA:
        assert_fma(tag, got, want32)
    else:
        G.assert_close(tag, np.asarray(got, F32).ravel(), np.asarray(want64, F64).ravel(), act_tol, rtol=act_tol,
                       afrac=act_tol / 10)


# ---- guarded device buffers -------------------------------------------------------------------------------------------------
BAND = 64                       # floats of sentinel on both sides of every view (a multiple of 4: views stay 16-byte aligned)
SENTINEL = 0x7FC0BEEF           # a quiet NaN with a payload: reading it into a result shows, writing over it shows
DEVICE = "cuda:0"


class Guarded:
    """A device tensor of `values.size` floats inside a larger allocation, BAND sentinel words before and after.
    `shift` floats of extra offset (1: a deliberately misaligned view). A zero-length view is legal."""

    def __init__(self, values, shift=0):
        import torch
        values = np.ascontiguousarray(np.asarray(values, F32)).ravel()
        self.n, self.start = values.size, BAND + shift
        total = self.start + self.n + BAND
        total += (-total) % 4
        host = np.full(total, SENTINEL, np.uint32)
        host[self.start:self.start + self.n] = values.view(np.uint32)
        self.host = host
        self.buf = torch.from_numpy(host.view(np.int32).copy()).to(DEVICE)
        assert self.buf.data_ptr() % 16 == 0                       # the allocation itself is 16-byte aligned
        self.ptr = self.buf.data_ptr() + 4 * self.start
        assert self.ptr % 16 == (4 * shift) % 16                   # "aligned" cases really are, misaligned ones really are not

    def read(self):
        """(values of the view as float32, copy) after asserting that both bands are bit-unchanged"""
        now = self.buf.cpu().numpy().view(np.uint32)
        lo, hi = now[:self.start], now[self.start + self.n:]
        assert np.array_equal(lo, self.host[:self.start]), "the band BEFORE the view was written"
        assert np.array_equal(hi, self.host[self.start + self.n:]), "the band AFTER the view was written"
        return now[self.start:self.start + self.n].copy().view(F32)

    def assert_unchanged(self, tag=""):
        """the whole view and both bands hold what was uploaded (an input, or an output the call must not touch)"""
        got = self.read()
        assert np.array_equal(got.view(np.uint32), self.host[self.start:self.start + self.n]), "%s: modified" % tag

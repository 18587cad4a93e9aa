"""The inputs, the float64 reference and the per-element bound of the attention tests (tests/test_attention_cases_host.py on the CPU,
tests/test_gpu_attention.py on the device).  CPU only: numpy, and torch for the 16-bit rounding.

One case is qkv [B * 192, 3 D].  The (crop, head) slab (b, h) gets scenario (b * heads + h) % 6, so every scenario sits on several heads and crops, in
the remapped block groups of head dim 32 / 80 and in their tail.  Every value is rounded to the operand type first.

    0 GAUSS    q x 1.5 Gaussian, one spiky query row: what tests/test_gpu_ops.py::test_attention draws
    1 ONEHOT   K rows = a seeded +-1 sign code, q_i = gain k_perm(i): the winning base-2 logit leads the runner-up by >= 140, so every other p rounds to 0
               (bf16 too: 2^-140 is below half its smallest subnormal), and out[i, :] == V[perm(i), :] exactly.  A row maximum taken over too few lanes
               leaves exp2 an argument >= 140: infinity, not a cancelling constant.
    2 FLAT     q = 0: every p is exactly 1, l = 192, out = the column mean of V; no P rounding takes part
    3 HOT      q = 12 (g + sign(c) / 2), every 7th query negated, K = g + c with c = +-3 per column: base-2 logits beyond +150 and rows whose maximum is <= -100
    4 MIXED    column d of V times 2^(d % 17 - 8), query i times 2^(i % 8 - 3): the case a bound against the global maximum cannot see
    5 EDGE     ONEHOT with edge values in V (+-65504 in fp16, +-2^100 in bf16, +-0, 2^-14) and TIE_PAIRS pairs of identical K rows: a query matched to one of
               a pair sees p = 1/2, 1/2 and out = (v_a + v_b) / 2, chosen representable

Domain.  fma(s, c, -fl(max c)) is not exactly 0 at the maximum, so p_max = 1 +- ulp(max c) / 2 ln 2.  At base-2 logits <= 2^10 (asserted for every case here)
that is 1 +- 2^-14.5 and the exact expectations hold with room (65504 (1 + 2^-14.5) < 65520); beyond about 2^13 a V value of 65504 could round to infinity
under the kernel's clamp-free output conversion.  The cases stay inside 2^10; the outside is not tested.

The sign of a zero is not pinned: a sum of +0 products and one -0 is +0, whatever V holds."""
import functools

import numpy as np
import torch

T = 192
N_SCEN = 6
GAUSS, ONEHOT, FLAT, HOT, MIXED, EDGE = range(N_SCEN)
NAMES = ('gauss', 'onehot', 'flat', 'hot', 'mixed', 'edge')
U = {'fp16': 2.0 ** -11, 'bf16': 2.0 ** -8}            # half an ulp of the 16-bit types, relative
LOG2E = 1.4426950408889634
GAP_MIN, LOGIT_MAX = 140.0, 1024.0
HOT_HIGH, HOT_LOW = 150.0, -100.0
GAINS = (112.0, 96.0, 80.0, 72.0, 64.0, 56.0, 48.0)    # candidates for ONEHOT's gain (all exact in both types), largest first
TIE_PAIRS = tuple((16 * t + 5, 16 * ((t + 5) % 12) + 9 + (t % 3)) for t in range(0, 12, 2))   # six (a, b) pairs, every key tile touched, no key twice


def round_to(x, dtype):
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    return t.to(torch.float16 if dtype == 'fp16' else torch.bfloat16).float().numpy()


def scenario_of(b, h, heads):
    return (b * heads + h) % N_SCEN


@functools.lru_cache(maxsize=None)
def perm():
    """a fixed permutation of the 192 keys without fixed points that maps no 16-key tile onto itself: i -> 37 i + 11 mod 192 (37 is odd and no multiple of 3)"""
    p = (37 * np.arange(T) + 11) % T
    assert len(set(p.tolist())) == T and (p != np.arange(T)).all()
    return p


def base2_logits(q, k):
    """float64 base-2 logits [192, 192] of one slab"""
    hd = q.shape[1]
    return (q.astype(np.float64) @ k.astype(np.float64).T) * (hd ** -0.5 * LOG2E)


@functools.lru_cache(maxsize=None)
def sign_code(hd, ties):
    """(K [192, hd] of +-1, gain) for ONEHOT (ties = False) and EDGE (ties = True: row b of every TIE_PAIRS pair repeats row a): the first seed and the largest
    gain at which the winner leads by GAP_MIN and no |base-2 logit| exceeds LOGIT_MAX.  The lead is 2 gain dmin hd^-1/2 log2(e) for the smallest Hamming
    distance dmin between distinct rows, the winner gain hd^1/2 log2(e): only the ratio 2 dmin / hd is the code's."""
    for seed in range(64):
        k = np.where(np.random.default_rng(1000 * hd + seed).integers(0, 2, (T, hd)) > 0, 1.0, -1.0).astype(np.float32)
        if ties:
            for a, b in TIE_PAIRS:
                k[b] = k[a]
        g = k.astype(np.float64) @ k.astype(np.float64).T
        same = g == hd
        expect = np.eye(T, dtype=bool)
        if ties:
            for a, b in TIE_PAIRS:
                expect[a, b] = expect[b, a] = True
        if not np.array_equal(same, expect):
            continue
        runner = np.where(same, -np.inf, g).max()
        for gain in GAINS:
            win = gain * hd * hd ** -0.5 * LOG2E
            if win <= LOGIT_MAX and gain * (hd - runner) * hd ** -0.5 * LOG2E >= GAP_MIN:
                return k, gain
    raise AssertionError(f'no sign code for head dim {hd}')


def _edge_values(dtype):
    big = 65504.0 if dtype == 'fp16' else 2.0 ** 100
    return np.array([big, -big, 0.0, -0.0, 2.0 ** -14, 1.5, -0.375], np.float32)


def build_slab(scen, dtype, hd, rng):
    """(q, k, v) [192, hd] float32, rounded to dtype"""
    g = lambda: rng.standard_normal((T, hd)).astype(np.float32)
    q, k, v = g(), g(), g()
    if scen == GAUSS:
        q *= 1.5
        q[5] *= 4.0
    elif scen in (ONEHOT, EDGE):
        k, gain = sign_code(hd, scen == EDGE)
        q = gain * k[perm()]
        if scen == EDGE:
            ev = _edge_values(dtype)
            v = round_to(v, dtype)
            pick = rng.integers(0, 2 * len(ev), (T, hd))            # half of V from the edge list
            v = np.where(pick < len(ev), ev[pick % len(ev)], v).astype(np.float32)
            mode = np.arange(hd) % 3                                 # tied rows: v_b = v_a, -v_a, 0 by column -> means v_a, 0, v_a / 2
            v[TIE_PAIRS[0][0], :3] = (ev[0], ev[0], ev[4])              # a saturated mean, a cancelled one, and 2^-15 (below fp16's smallest normal)
            for a, b in TIE_PAIRS:
                v[b] = np.where(mode == 0, v[a], np.where(mode == 1, -v[a], 0.0))
    elif scen == FLAT:
        q[:] = 0.0
    elif scen == HOT:
        c = np.where(rng.integers(0, 2, hd) > 0, 3.0, -3.0).astype(np.float32)
        q = 12.0 * (q + 0.5 * np.sign(c))
        q[::7] *= -1.0
        k = k + c
    elif scen == MIXED:
        v *= np.exp2(np.arange(hd) % 17 - 8).astype(np.float32)
        q *= np.exp2(np.arange(T) % 8 - 3).astype(np.float32)[:, None]
    return round_to(q, dtype), round_to(k, dtype), round_to(v, dtype)


class Case:
    """qkv [B 192, 3 D] float32 (rounded to dtype) and, per element of the output [B 192, D]: ref, mag, the scenario; per row and head: lam"""

    def __init__(self, dtype, B, D, heads, seed=0):
        self.dtype, self.B, self.D, self.heads, self.hd = dtype, B, D, heads, D // heads
        hd = self.hd
        rng = np.random.default_rng(7919 * D + 31 * heads + seed)
        M = B * T
        self.qkv = np.empty((M, 3 * D), np.float32)
        self.ref = np.empty((M, D), np.float64)
        self.mag = np.empty((M, D), np.float64)
        self.sub = np.empty((M, D), np.float64)          # sum |v_kj| / l over the keys whose p is below the 16-bit type's normal range
        self.lam = np.empty((M, heads), np.float64)
        self.scen = np.empty((B, heads), np.int64)
        self.logit_max = np.empty((B, heads, T))       # per query: the largest base-2 logit
        self.logit_abs = 0.0
        for b in range(B):
            for h in range(heads):
                s = scenario_of(b, h, heads)
                self.scen[b, h] = s
                q, k, v = build_slab(s, dtype, hd, rng)
                rows, cols = slice(b * T, (b + 1) * T), slice(h * hd, (h + 1) * hd)
                for i, x in enumerate((q, k, v)):
                    self.qkv[rows, i * D + h * hd:i * D + (h + 1) * hd] = x
                self.ref[rows, cols], self.mag[rows, cols], self.lam[rows, h], lg, self.sub[rows, cols] = reference(q, k, v, dtype)
                self.logit_max[b, h] = lg.max(1)
                self.logit_abs = max(self.logit_abs, np.abs(lg).max())
        self.scen_el = np.repeat(np.repeat(self.scen, T, axis=0), hd, axis=1)          # [M, D]

    def slab(self, b, h):
        rows, hd, D = slice(b * T, (b + 1) * T), self.hd, self.D
        return tuple(self.qkv[rows, i * D + h * hd:i * D + (h + 1) * hd] for i in range(3))

    def slabs(self, scen):
        return [(b, h) for b in range(self.B) for h in range(self.heads) if self.scen[b, h] == scen]

    def bound(self):
        """the per-element bound [M, D]; FLAT slabs without the P-rounding term"""
        lam = np.repeat(self.lam, self.hd, axis=1)
        return bound(self.dtype, self.ref, self.mag, lam, self.sub, p_rounding=self.scen_el != FLAT)

    def exact(self):
        """(mask [M, D], expected [M, D] float32) of the elements whose value is known exactly: ONEHOT, EDGE"""
        mask = np.zeros(self.ref.shape, bool)
        exp = np.zeros(self.ref.shape, np.float32)
        for s in (ONEHOT, EDGE):
            for b, h in self.slabs(s):
                rows, cols = slice(b * T, (b + 1) * T), slice(h * self.hd, (h + 1) * self.hd)
                mask[rows, cols] = True
                exp[rows, cols] = expected_exact(s, self.slab(b, h)[2])
        return mask, exp


P_NORMAL = {'fp16': 2.0 ** -14, 'bf16': 2.0 ** -126}   # the smallest normal of the type P is rounded to


def reference(q, k, v, dtype):
    """float64 softmax(q k^T hd^-1/2) v of one slab -> ref [192, hd], mag = sum_k p |v|, lam [192] = max_j hd^-1/2 sum_d |q_d k_jd|, the base-2 logits, and
    sub = sum |v_kj| / l over the keys whose unnormalised p = exp(s - max) is below twice the smallest normal of dtype (twice: p is known to fp32 accuracy only)"""
    hd = q.shape[1]
    q, k, v = (x.astype(np.float64) for x in (q, k, v))
    s = (q @ k.T) * hd ** -0.5
    p = np.exp(s - s.max(1, keepdims=True))
    l = p.sum(1, keepdims=True)
    sub = ((p < 2 * P_NORMAL[dtype]) / l) @ np.abs(v)
    p /= l
    lam = (np.abs(q) @ np.abs(k).T).max(1) * hd ** -0.5
    return p @ v, p @ np.abs(v), lam, s * LOG2E, sub


def bound(dtype, ref, mag, lam, sub, p_rounding=True):
    """|got - ref| <= u |ref| (the output rounding) + u mag (P rounded to 16 bits before PV) + 2^-24 (8 + lam) mag (fp32 accumulation of S and PV, the
    exponent's argument) + eta (1 + sub p_rounding): where the 16-bit type stops being a RELATIVE format.  From the kernel's roundings alone; nothing in it is
    fitted to the kernel's result.

    eta, fp16: 2^-25, half the spacing of its subnormals.  An output below 2^-14 is rounded to that grid (the 1), and so is a p below 2^-14: the u mag term
    takes |P~ - p| <= u p, which holds for normal p only; each smaller p adds up to 2^-25 |v_kj| / l instead (sub).  Hot logits with V of the order of 10^3 reach
    this: the float32 model of the kernel exceeds the relative terms alone by 1.5 x on the fused kernels' operands, on outputs that are fp16 subnormals.
    eta, bf16: 2^-126, its smallest normal (bf16 has fp32's exponent range): a p or an output below it may become 0 -- the exponential's result, the conversion, the
    MFMA's operand.  With V values of 2^100 beside zeros (EDGE) the float64 reference of an output that is exactly 0 in any 16-bit arithmetic is 2^100 2^-gap > 0."""
    u = U[dtype]
    eta = 2.0 ** -25 if dtype == 'fp16' else 2.0 ** -126
    return u * np.abs(ref) + u * mag * p_rounding + 2.0 ** -24 * (8.0 + lam) * mag + eta * (1.0 + sub * p_rounding)


def expected_exact(scen, v):
    """ONEHOT / EDGE: the exact output [192, hd] of a slab with values v"""
    p = perm()
    out = v[p].astype(np.float64)
    if scen == EDGE:
        partner = {a: b for a, b in TIE_PAIRS}
        partner.update({b: a for a, b in TIE_PAIRS})
        for i in range(T):
            if p[i] in partner:
                out[i] = (v[p[i]].astype(np.float64) + v[partner[p[i]]].astype(np.float64)) / 2
    return out.astype(np.float32)


def check_conditions(case):
    """the conditions the scenarios promise, in float64; raises AssertionError.  Run before any device call."""
    assert case.logit_abs <= LOGIT_MAX, f'|base-2 logit| {case.logit_abs} beyond {LOGIT_MAX}'
    for s in range(N_SCEN):
        assert len(case.slabs(s)) >= 2, f'scenario {s} on fewer than two slabs'
    p = perm()
    for s in (ONEHOT, EDGE):
        for b, h in case.slabs(s):
            q, k, v = case.slab(b, h)
            lg = base2_logits(q, k)
            assert np.abs(lg).max() <= LOGIT_MAX
            win = lg[np.arange(T), p]
            tied = lg == win[:, None]                                         # exact: the logits are integers times one constant
            rest = np.where(tied, -np.inf, lg).max(1)
            assert (win == lg.max(1)).all() and (win - rest >= GAP_MIN).all(), f'lead {np.min(win - rest)}'
            assert (tied.sum(1) == 1 + (s == EDGE) * np.isin(p, np.array(TIE_PAIRS).ravel())).all()      # the argmax is perm, alone or with its twin
            exp = expected_exact(s, v)
            assert np.array_equal(round_to(exp, case.dtype), exp), 'an expected value is not representable'
            if s == EDGE:
                big = _edge_values(case.dtype)[0]
                for val in (big, -big, 2.0 ** -14):
                    assert (exp == val).any(), f'{val} is not among the expected outputs'
                assert (exp == 0).any() and (np.signbit(v) & (v == 0)).any()
                assert (exp == 2.0 ** -15).any()                               # a tie mean below the smallest normal of fp16
    for b, h in case.slabs(FLAT):
        assert not case.slab(b, h)[0].any()
    for b, h in case.slabs(HOT):
        assert case.logit_max[b, h].max() >= HOT_HIGH and case.logit_max[b, h].min() <= HOT_LOW, (case.logit_max[b, h].max(), case.logit_max[b, h].min())
    for b, h in case.slabs(MIXED):
        v = np.abs(case.slab(b, h)[2]).max(0)
        assert v.max() / v.min() >= 2.0 ** 14


@functools.lru_cache(maxsize=None)
def case(dtype, B, D, heads):
    """the shared case of a shape: built once, never written to"""
    c = Case(dtype, B, D, heads)
    for a in (c.qkv, c.ref, c.mag, c.lam, c.sub):
        a.setflags(write=False)
    return c


def worst_ratio(case, got):
    """{scenario name: max |got - ref| / bound} (inf where got is not finite)"""
    with np.errstate(invalid='ignore'):
        ratio = np.where(np.isfinite(got), np.abs(got.astype(np.float64) - case.ref) / case.bound(), np.inf)
    return {NAMES[s]: float(ratio[case.scen_el == s].max()) for s in range(N_SCEN)}


# ---------------------------------------------------------------- the fused kernels' operands (vp_dbg_qkvattn: x [M, D], W [3 D, D], bias [3 D])
def fused_operands(dtype, D, heads, npairs):
    """Hot operands for attn.qkv + attention in one kernel: the q rows of W at 12x, outlier channels in x.  One head-dim channel per head (d = 3) carries a k
    and a v that leave the fp16 range on the outlier tokens (the hand-over to the attention phase saturates them); the q rows of that channel are zero with a
    zero bias, so the saturated k multiplies an exact 0 and the logits stay inside LOGIT_MAX."""
    M, hd = npairs * 384, D // heads
    rng = np.random.default_rng(3 * D + npairs)
    x = rng.standard_normal((M, D)).astype(np.float32)
    out_ch = np.arange(5, D, 97)
    x[:, out_ch] *= 6.0
    x[::5, out_ch[0]] = 250.0                                        # the outlier tokens
    W = (rng.standard_normal((3 * D, D)) * (1.5 / np.sqrt(D))).astype(np.float32)
    W[:D] *= 12.0
    bias = (0.1 * rng.standard_normal(3 * D)).astype(np.float32)
    W[:, out_ch[0]] = 0.0                                              # the outlier tokens stay ordinary in every other channel
    sat = np.arange(heads) * hd + 3
    W[sat] = 0.0
    bias[sat] = 0.0
    W[D + sat, out_ch[0]] = 300.0
    W[2 * D + sat, out_ch[0]] = -290.0
    return round_to(x, dtype), round_to(W, dtype), bias


def fused_qkv64(dtype, x, W, bias):
    """x W^T + b in float64, and the same as the hand-over stores it (fp16: saturated at +-65504)"""
    full = (torch.from_numpy(x).double() @ torch.from_numpy(W).double().T).numpy() + bias.astype(np.float64)
    stored = round_to(np.clip(full, -65504.0, 65504.0) if dtype == 'fp16' else full, dtype)
    return full, stored


def check_fused_conditions(dtype, D, heads, full, stored):
    hd, M = D // heads, full.shape[0]
    if dtype == 'fp16':
        assert (np.abs(full[:, D:2 * D]) > 65504).any() and (np.abs(full[:, 2 * D:]) > 65504).any(), 'no value beyond the fp16 range in k and v'
    hot = 0
    top = -np.inf
    for b in range(M // T):
        for h in range(heads):
            q, k = (stored[b * T:(b + 1) * T, i * D + h * hd:i * D + (h + 1) * hd] for i in range(2))
            lg = base2_logits(q, k)
            assert np.abs(lg).max() <= LOGIT_MAX, np.abs(lg).max()
            top = max(top, lg.max())
            srt = np.sort(lg, axis=1)
            hot += (np.exp2(srt[:, :-1] - srt[:, -1:]).sum(1) <= 1 / 0.99 - 1).sum()
    print(f'[fused operands] {dtype} D={D}: largest base-2 logit {top:.0f}, {hot} of {M * heads} queries with max p >= 0.99')
    assert top >= HOT_HIGH, top
    assert hot >= M * heads / 4, f'{hot} of {M * heads} queries with max p >= 0.99'

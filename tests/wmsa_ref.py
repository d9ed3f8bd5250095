"""numpy float64 restatement of the W-MSA attention core (oracle/swinv2_ref.py::wmsa_core_ref and
its autograd gradients), written window by window with the pieces exposed: the reference of
tests/test_wmsa_ref_cpu.py and tests/test_gpu_wmsa_blocks.py.

core(...) returns the output, the four gradients, the absolute-sum "sizes" that the
per-entry comparisons divide by, and the gather map, so a test can cut any [B, L, C] tensor into
(image, window, head) blocks.  unit_errors(...) is the comparison itself: one normalised error per
block / table entry / head / channel, none left out.

round_ops=True is the honest-bf16 baseline: the same float64 math with a round-to-nearest-even bf16
rounding of exactly the operands the kernels hand to the MFMA, and of the bf16 outputs out and
dqkv.  Accumulation order, exp2 against exp, f32 row statistics and everything else a kernel
does are NOT modelled.  The rounded operands, read from the kernels (hierarchical-vision_amd/csrc):

forward, every form (wmsa_win.hip, wmsa_ring.hip, wmsa_large.hip)
  q image  bf16(q^ * scale * log2e)          wmsa_win.hip:317, wmsa_ring.hip:292, wmsa_large.hip:246
  k image  bf16(k^)                          wmsa_win.hip:318, wmsa_ring.hip:293, wmsa_large.hip:237
  P        bf16(exp2(S' - M_h)), NOT normalised, M_h = log2e (scale + max bias) the head bound
           (the row max where the row sum falls below 2^-100); the row sum is taken over the same
           rounded P by a ones-vector MFMA      wmsa_win.hip:377-381, wmsa_ring.hip:338,
                                               wmsa_large.hip:348 (HVK_FWD_ROWSUM_MFMA, :25)
  V        bf16 as given
  out      bf16((P V) / sum P)                 wmsa_win.hip:439, wmsa_ring.hip:415, wmsa_large.hip:467

backward, form "small" (wmsa.hip, w <= 8, raw q / k)
  q, k images  bf16(q^), bf16(k^)              wmsa.hip:390-391; cos = q^ . k^ in f32 (:435)
  dO, V        bf16 as given (dP = dO . V, :436)
  P            bf16(P), normalised, for dV     wmsa.hip:521
  scale * dS   bf16, for dQ^ and dK^           wmsa.hip:515-516; the f32 value feeds the table and
                                               logit-scale sums (:512-513)
  the normalisation's backward projects with the ROUNDED q^ / k^ images   wmsa.hip:538, :602
  dq, dk, dv   bf16                            wmsa.hip:556, :619-620; dq_bias sums the f32 dq (:554)

backward, form "normed" (wmsa.hip with BwdArgs::rn, the hvk_wmsa_*_normed entries): as "small" but
  the q image is bf16(q^ * scale * log2e), made by hvk_qk_normalize / the qkv GEMM epilogue
  (wmsa.hip:450, :545: cos and the projection divide the factor out again)

backward, form "large" (wmsa_large.hip, w = 12 / 16 / 24)
  q image      bf16(q^ * scale * log2e)        wmsa_large.hip:745, :619 (write_rows)
  k image      bf16(k^)                        wmsa_large.hip:950, :619
  P            bf16(P), normalised, for dV     wmsa_large.hip:1029
  dS           bf16, WITHOUT the scale         wmsa_large.hip:880, :1031
  the normalisation's backward uses the f32 x * rn, not the image   wmsa_large.hip:534-551
  dq, dk, dv   bf16                            wmsa_large.hip:551, :1046
  The row constants are modelled as exact (the recomputing backward, wmsa_large_lse off); with
  them taken from the forward, delta = dO . O is corrected by loop B's own row sums (:896-910).
"""
import numpy as np

from oracle import index_ref

LOG2E = 1.4426950408889634
EPS = 1e-12
FORMS = ("small", "normed", "large")
CLASSES = ("out", "dq", "dk", "dv", "dbias", "dscale", "dq_bias")


def default_form(win):
    return "small" if win <= 8 else "large"


def _np(x):
    if hasattr(x, "detach"):
        x = x.detach().cpu().double().numpy()
    return np.asarray(x, np.float64)


def bf16(x):
    """Round-to-nearest-even to bf16 (through float32), returned as float64."""
    u = np.ascontiguousarray(np.asarray(x, np.float64).astype(np.float32)).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).astype(np.float64)


def _softmax(s):
    e = np.exp(s - s.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def _t(x):
    return np.swapaxes(x, -1, -2)


def _normalize_bwd(dxh, xh, norm):
    """Backward of x / max(||x||, eps): (dx^ - x^ (x^ . dx^)) / ||x||, and dx^ / eps without the
    projection where ||x|| <= eps."""
    tiny = norm <= EPS
    dot = np.where(tiny, 0.0, (xh * dxh).sum(-1, keepdims=True))
    return (dxh - xh * dot) / np.maximum(norm, EPS)


def core(qkv, table, scale, H, W, nh, win, shift, gout=None, round_ops=False, form=None):
    """qkv [B, H*W, 3C], table [nh, (2w-1)^2], scale [nh], gout [B, H*W, C] or None.  Returns a
    dict: out [B, L, C]; with gout dqkv [B, L, 3C], dbias [nh, RR], dscale [nh], dq_bias [C] and
    the sizes size_dbias [nh, RR] = sum |dS_ij| over every (image, window, query, key) pair of the
    entry, size_dscale [nh] = sum |dS_ij cos_ij|, size_dq_bias [C] = sum over tokens |dq| (always
    from the exact math, also with round_ops); g [nW, n] the gather map."""
    qkv, table, scale = _np(qkv), _np(table), _np(scale)
    form = form or default_form(win)
    assert form in FORMS, form
    B, L, C3 = qkv.shape
    C = C3 // 3
    d = C // nh
    assert L == H * W and C == nh * d
    g = index_ref.window_gather_map(H, W, win, shift).astype(np.int64)
    nW, n = g.shape
    rpi = index_ref.relative_position_index(win)
    RR = (2 * win - 1) ** 2
    m = index_ref.shift_mask(H, W, win, shift)
    mask = 0.0 if m is None else m.astype(np.float64)[:, None]          # [nW, 1, n, n]
    bias = table[:, rpi.reshape(-1)].reshape(1, nh, n, n)
    sc = scale.reshape(1, nh, 1, 1)
    sc2 = sc * LOG2E
    bin_idx = (np.arange(nh)[:, None, None] * RR + rpi[None]).reshape(-1)  # [nh n n]

    res = {"g": g, "out": np.empty((B, L, C))}
    if gout is not None:
        gout = _np(gout)
        res.update(dqkv=np.empty((B, L, C3)), dbias=np.zeros((nh, RR)), dscale=np.zeros(nh),
                   dq_bias=np.zeros(C), size_dbias=np.zeros((nh, RR)), size_dscale=np.zeros(nh),
                   size_dq_bias=np.zeros(C))

    def heads(x):  # [nW, n, C] -> [nW, nh, n, d]
        return x.reshape(nW, n, nh, d).transpose(0, 2, 1, 3)

    def tokens(x):  # back
        return x.transpose(0, 2, 1, 3).reshape(nW, n, C)

    def bins(x):  # [nW, nh, n, n] -> [nh, RR]
        return np.bincount(bin_idx, weights=x.sum(0).reshape(-1), minlength=nh * RR).reshape(nh, RR)

    for b in range(B):
        x = qkv[b][g]                                                     # [nW, n, 3C]
        q, k, v = (heads(x[..., i * C:(i + 1) * C]) for i in range(3))
        nq = np.sqrt((q * q).sum(-1, keepdims=True))
        nk = np.sqrt((k * k).sum(-1, keepdims=True))
        qh, kh = q / np.maximum(nq, EPS), k / np.maximum(nk, EPS)

        # ---- exact
        cos = qh @ _t(kh)
        P = _softmax(cos * sc + bias + mask)
        if not round_ops:
            o = P @ v
        else:
            qi, ki = bf16(qh * sc2), bf16(kh)
            s2 = qi @ _t(ki) + (bias + mask) * LOG2E
            Mh = (scale + table.max(1)).reshape(1, nh, 1, 1) * LOG2E
            Pu = bf16(np.exp2(s2 - Mh))
            low = Pu.sum(-1, keepdims=True) < 2.0 ** -100
            if low.any():
                Pu = np.where(low, bf16(np.exp2(s2 - s2.max(-1, keepdims=True))), Pu)
            o = bf16((Pu @ v) / Pu.sum(-1, keepdims=True))
        res["out"][b][g] = tokens(o)
        if gout is None:
            continue

        dO = heads(gout[b][g])
        dp = dO @ _t(v)
        dS = P * (dp - (P * dp).sum(-1, keepdims=True))
        dq_exact = _normalize_bwd(sc * (dS @ kh), qh, nq)
        res["size_dbias"] += bins(np.abs(dS))
        res["size_dscale"] += np.abs(dS * cos).sum((0, 2, 3))
        res["size_dq_bias"] += np.abs(tokens(dq_exact)).sum((0, 1))
        if not round_ops:
            dq = dq_exact
            dk = _normalize_bwd(sc * (_t(dS) @ qh), kh, nk)
            dv = _t(P) @ dO
            dq_sum = dq
        else:
            qi = bf16(qh * sc2) / sc2 if form in ("normed", "large") else bf16(qh)
            ki = bf16(kh)
            cos = qi @ _t(ki)
            P = _softmax(cos * sc + bias + mask)
            dS = P * (dp - (P * dp).sum(-1, keepdims=True))
            dsr = bf16(dS) if form == "large" else bf16(dS * sc) / sc
            qp, kp = (qh, kh) if form == "large" else (qi, ki)
            dq_sum = _normalize_bwd(sc * (dsr @ ki), qp, nq)
            dq = bf16(dq_sum)
            dk = bf16(_normalize_bwd(sc * (_t(dsr) @ qi), kp, nk))
            dv = bf16(_t(bf16(P)) @ dO)
        res["dbias"] += bins(dS)
        res["dscale"] += (dS * cos).sum((0, 2, 3))
        res["dq_bias"] += tokens(dq_sum).sum((0, 1))
        res["dqkv"][b][g] = np.concatenate([tokens(dq), tokens(dk), tokens(dv)], -1)
    return res


# --------------------------------------------------------------------------- comparison
def _ratio(err, size):
    """err / size per unit; a unit of size 0 must be matched exactly (else inf)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(size > 0, err / np.where(size > 0, size, 1.0), np.where(err > 0, np.inf, 0.0))


def block_norms(x, g, nh):
    """[B, L, C] -> [B, nW, nh] Frobenius norms of the (image, window, head) blocks, n x C/nh."""
    x = np.asarray(x, np.float64)
    B, _, C = x.shape
    nW, n = g.shape
    xb = x[:, g].reshape(B, nW, n, nh, C // nh)
    return np.sqrt((xb * xb).sum((2, 4)))


def unit_errors(got, ref, nh, classes=None):
    """One normalised error per unit of each class: `got` holds out / dqkv / dbias / dscale /
    dq_bias (any subset), `ref` is core(round_ops=False) on the same inputs.
      out, dq, dk, dv  [B, nW, nh]  ||got - ref|| / ||ref|| of the block
      dbias            [nh, RR]     |got - ref| / sum |dS| of the entry
      dscale           [nh]         |got - ref| / sum |dS cos|
      dq_bias          [C]          |got - ref| / sum |dq|"""
    g = ref["g"]
    C = ref["out"].shape[-1]
    errs = {}
    if "out" in got:
        errs["out"] = _ratio(block_norms(_np(got["out"]) - ref["out"], g, nh), block_norms(ref["out"], g, nh))
    if "dqkv" in got:
        dqkv = _np(got["dqkv"])
        for i, name in enumerate(("dq", "dk", "dv")):
            r = ref["dqkv"][..., i * C:(i + 1) * C]
            errs[name] = _ratio(block_norms(dqkv[..., i * C:(i + 1) * C] - r, g, nh), block_norms(r, g, nh))
    for name in ("dbias", "dscale", "dq_bias"):
        if name in got:
            errs[name] = _ratio(np.abs(_np(got[name]) - ref[name]), ref["size_" + name])
    if classes is not None:
        errs = {k: v for k, v in errs.items() if k in classes}
    return errs


def worst(errs):
    """{class: (worst normalised error, index of that unit)}."""
    return {k: (float(v.max()), tuple(int(i) for i in np.unravel_index(int(v.argmax()), v.shape)))
            for k, v in errs.items()}


def whole_tensor_rel(got, ref):
    """The figures of tests/test_gpu_wmsa.py: ||got - ref|| / ||ref|| over each whole tensor."""
    out = {}
    for name in ("out", "dqkv", "dbias", "dscale", "dq_bias"):
        if name in got:
            out[name] = float(np.linalg.norm(_np(got[name]) - ref[name]) / max(np.linalg.norm(ref[name]), 1e-300))
    return out


WHOLE_BOUNDS = {"out": 1e-2, "dqkv": 2e-2, "dbias": 2e-2, "dscale": 5e-2, "dq_bias": 2e-2}
FACTOR = 2.0  # observed worst unit <= FACTOR x the baseline's worst unit, per class


def describe_unit(name, idx, H, W, win, shift):
    """Where a unit sits: for a block its image, window row / column, head and mask class."""
    if name in ("out", "dq", "dk", "dv"):
        b, k, h = idx
        nWw = W // win
        wh, ww = divmod(k, nWw)
        edge = ("r" if shift and wh == H // win - 1 else "") + ("c" if shift and ww == nWw - 1 else "")
        return f"image {b} window {k} (row {wh}, col {ww}, mask {edge or 'none'}) head {h}"
    if name == "dbias":
        h, e = idx
        dy, dx = divmod(e, 2 * win - 1)
        return f"head {h} offset ({dy - win + 1}, {dx - win + 1})"
    return f"{'head' if name == 'dscale' else 'channel'} {idx[0]}"


def check_units(got, ref, base, nh, geom=None):
    """(table rows, failures): per class the observed and the baseline worst unit and their ratio;
    a class fails when observed > FACTOR x baseline.  `base` is core(round_ops=True)."""
    obs = worst(unit_errors(got, ref, nh))
    bas = worst(unit_errors(base, ref, nh, classes=obs.keys()))
    rows, bad = [], []
    for name in CLASSES:
        if name not in obs:
            continue
        o, oi = obs[name]
        bl, _ = bas[name]
        where = describe_unit(name, oi, *geom) if geom else str(oi)
        rows.append((name, o, bl, o / bl if bl > 0 else (0.0 if o == 0 else float("inf")), where))
        if not o <= FACTOR * bl:
            bad.append(rows[-1])
    return rows, bad


def format_rows(case, rows):
    return [f"{case:<34s} {name:<8s} observed {o:.3e}  baseline {bl:.3e}  ratio {r:5.2f}  worst: {where}"
            for name, o, bl, r, where in rows]


# --------------------------------------------------------------------------- inputs
def inputs(B, H, W, nh, win, seed, std=1.0):
    """The _inputs recipe of tests/test_gpu_wmsa.py in numpy: bf16-representable qkv, table
    16 sigmoid(.), scale about 10 (float32 values held in float64)."""
    rng = np.random.default_rng(seed)
    C = 32 * nh
    qkv = bf16((std * rng.standard_normal((B, H * W, 3 * C))).astype(np.float32))
    tab = (16 / (1 + np.exp(-rng.standard_normal((nh, (2 * win - 1) ** 2))))).astype(np.float32).astype(np.float64)
    scale = np.exp(np.minimum(np.log(10) + 0.5 * rng.standard_normal(nh), np.log(100))).astype(np.float32)
    return qkv, tab, scale.astype(np.float64)


def grad_out(B, H, W, nh, seed):
    rng = np.random.default_rng(seed)
    return bf16(rng.standard_normal((B, H * W, 32 * nh)).astype(np.float32))


# --------------------------------------------------------------------------- geometry pin
PIN_V, PIN_G = 8.0, 4.0       # max |v|, max |gout| of the codes
PIN_TOL = 2.0 ** -6           # x max |v| (out) or max |gout| (dv), elementwise


def _code(H, W, C, amp, rev):
    """[H*W, C] two-level code +-amp: channel c carries bit (c mod 12) of the 12-bit position word
    y * 64 + x (`rev`: x * 64 + y), inverted on every other run of 12 channels.  Any two tokens
    differ in some bit, so in some channel of every head (32 > 12) by the full 2 amp: the largest
    step a code of maximum `amp` can have, which is what the tolerance 2^-6 amp is measured
    against; neighbours differ in bit 0 of x or y."""
    y, x = np.divmod(np.arange(H * W), W)
    word = (x * 64 + y) if rev else (y * 64 + x)
    c = np.arange(C)
    bit = (word[:, None] >> (c % 12)[None, :]) & 1
    return amp * (1.0 - 2.0 * (bit ^ ((c // 12) & 1)[None, :]))


def pin_inputs(B, H, W, nh, win, seed):
    """Near-uniform attention: table 0, scale 1e-3, random q / k, coded v and gout.  The softmax is
    uniform over the unmasked members of a window to within 2e-3, so out and dv are region means
    of the codes: exactly what partition, roll and mask decide."""
    rng = np.random.default_rng(seed)
    C = 32 * nh
    qk = bf16(rng.standard_normal((B, H * W, 2 * C)).astype(np.float32))
    v = np.broadcast_to(_code(H, W, C, PIN_V, False), (B, H * W, C))
    qkv = np.concatenate([qk, v], -1)
    gout = np.broadcast_to(_code(H, W, C, PIN_G, True), (B, H * W, C)).copy()
    return qkv, np.zeros((nh, (2 * win - 1) ** 2)), np.full(nh, 1e-3), gout


def pin_excess(got_out, got_dqkv, ref):
    """(worst |out - out64| / (tol max|v|), worst |dv - dv64| / (tol max|gout|)): <= 1 passes."""
    C = ref["out"].shape[-1]
    eo = np.abs(_np(got_out) - ref["out"]).max() / (PIN_TOL * PIN_V)
    ev = np.abs(_np(got_dqkv)[..., 2 * C:] - ref["dqkv"][..., 2 * C:]).max() / (PIN_TOL * PIN_G)
    return float(eo), float(ev)


# --------------------------------------------------------------------------- the block cases
# (group, (B, H, W, heads, window, shift), backward form): tests/test_gpu_wmsa_blocks.py runs every
# one on the GPU, tools/wmsa_baseline_blocks.py tabulates their baselines
BLOCK_CASES = [
    # all four mask classes in one image, each form and window size; nWh != nWw; unshifted
    ("mask", (1, 14, 14, 1, 7, 3), "small"), ("mask", (1, 14, 14, 3, 7, 3), "small"),
    ("mask", (1, 21, 14, 3, 7, 3), "small"), ("mask", (1, 16, 16, 2, 8, 4), "small"),
    ("mask", (1, 12, 12, 4, 6, 3), "small"), ("mask", (1, 8, 8, 2, 4, 2), "small"),
    ("mask", (2, 7, 7, 24, 7, 0), "small"),
    # windows that do not divide evenly over the chunks: 24 over 512 / 24 = 21 slots, 192 over 170
    ("split", (4, 14, 21, 24, 7, 3), "small"), ("split", (3, 56, 56, 3, 7, 3), "small"),
    # batch slices of two images + 17 bytes: a short last slice that adds into the slots
    ("slices", (5, 14, 14, 2, 7, 3), "small"),
    # large windows: geometry, then more windows than chunks at 32 heads (256 / 32 = 8 chunks)
    ("large", (1, 24, 24, 2, 12, 6), "large"), ("large", (1, 32, 32, 2, 16, 8), "large"),
    ("large", (1, 48, 48, 2, 24, 12), "large"), ("large", (9, 12, 12, 32, 12, 0), "large"),
    ("large", (3, 24, 24, 32, 12, 6), "large"),
    # hvk_wmsa_fwd_normed / hvk_wmsa_bwd_normed
    ("normed", (1, 14, 14, 3, 7, 3), "normed"), ("normed", (1, 16, 16, 2, 8, 4), "normed"),
]
SEED_IN, SEED_GOUT = 21, 22


def case_id(group, geom):
    return group + "-" + "x".join(str(v) for v in geom)


_CASE_CACHE = {}


def block_case(group, geom, form):
    """(qkv, table, scale, gout, ref, base) of a block case, computed once per process and shared:
    ref = core(round_ops=False), base = core(round_ops=True, form)."""
    key = (geom, form)
    if key not in _CASE_CACHE:
        B, H, W, nh, win, shift = geom
        qkv, tab, scale = inputs(B, H, W, nh, win, SEED_IN)
        gout = grad_out(B, H, W, nh, SEED_GOUT)
        ref = core(qkv, tab, scale, H, W, nh, win, shift, gout)
        base = core(qkv, tab, scale, H, W, nh, win, shift, gout, round_ops=True, form=form)
        _CASE_CACHE[key] = (qkv, tab, scale, gout, ref, base)
    return _CASE_CACHE[key]


def baseline_rows(group, geom, form):
    """[(class, worst normalised error of the baseline, where)] of one block case."""
    _, _, _, _, ref, base = block_case(group, geom, form)
    B, H, W, nh, win, shift = geom
    w = worst(unit_errors(base, ref, nh))
    return [(name, w[name][0], describe_unit(name, w[name][1], H, W, win, shift)) for name in CLASSES]

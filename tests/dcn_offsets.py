"""Structured sampling offsets for the deformable-convolution tests (helper, no tests).

A continuous Gaussian draw never puts a sampling coordinate on an integer, on a validity edge
(h = -1, 0, H-1, H), on a window margin or far outside the image -- the places where the values
decide the samplers' control flow.  ``structured_offsets`` builds offsets whose every sample
(pixel, tap, deformable group) belongs to one such class, chosen by a seeded draw so that every
tile of every kernel holds a mix; ``masked_equivalent`` is the reference construction for the
samples the CPU oracle cannot be called on (its ``(int)ih`` is undefined past 2^31).

The sampling coordinate is ONE fp32 add, h = float(base_h) + off_h (mdcn_common.h:5), with
base_h = ho * stride - pad + i * dil; ``sample_coords`` restates it.
"""
import numpy as np

CLASSES = ("zero", "int", "half", "edge", "ulp", "margin", "far", "nan")
CID = {name: i for i, name in enumerate(CLASSES)}
# classes whose coordinates are exactly representable: the float64 oracle sees the kernel's own
# coordinate (for `margin` through coord_offsets64, see there)
EXACT = ("zero", "int", "half", "edge", "margin")

F32 = np.float32
_NEG2_OUT = np.nextafter(F32(-2), F32(-np.inf))   # first value below the window margin
_POS2_IN = np.nextafter(F32(2), F32(0))           # last value inside it
MARGIN_VALUES = np.array([-2.0, _NEG2_OUT, _POS2_IN, 2.0, 2.5, -3.0], F32)
FAR_VALUES = np.array([17, -17, 40, -40, 1e4, -1e4, 1e9, -1e9, 3e38, -3e38, np.inf, -np.inf], F32)
# the far values the CPU oracle can be called on ((int)ih defined): the construction's own pin
FAR_VALUES_ORACLE = np.array([17, -17, 40, -40, 1e4, -1e4, 1e6, -1e6], F32)


def _ksize(K):
    k = int(round(K ** 0.5))
    assert k * k == K, K
    return k


def base_coords(K, Ho, Wo, stride, pad, dil):
    """(base_h [K, Ho, 1], base_w [K, 1, Wo]) as integers: the tap's undeformed position."""
    k = _ksize(K)
    taps = np.arange(K)
    bh = np.arange(Ho)[None, :, None] * stride - pad + (taps // k)[:, None, None] * dil
    bw = np.arange(Wo)[None, None, :] * stride - pad + (taps % k)[:, None, None] * dil
    return bh, bw


def split_offsets(off, dg, K):
    """off [N, dg*2*K, Ho, Wo] -> views (off_h, off_w) of shape [N, dg, K, Ho, Wo]."""
    N, _, Ho, Wo = off.shape
    v = off.reshape(N, dg, K, 2, Ho, Wo)
    return v[:, :, :, 0], v[:, :, :, 1]


def sample_coords(off, dg, K, stride, pad, dil):
    """The kernels' fp32 sampling coordinates (h, w), each [N, dg*K, Ho, Wo]."""
    N, _, Ho, Wo = off.shape
    bh, bw = base_coords(K, Ho, Wo, stride, pad, dil)
    oh, ow = split_offsets(np.asarray(off, F32), dg, K)
    with np.errstate(invalid="ignore", over="ignore"):
        h = (bh.astype(F32)[None, None] + oh).astype(F32)
        w = (bw.astype(F32)[None, None] + ow).astype(F32)
    return h.reshape(N, dg * K, Ho, Wo), w.reshape(N, dg * K, Ho, Wo)


def invalid_samples(off, dg, K, H, W, stride, pad, dil):
    """Samples that are invalid in the oracle's sense (oracle_impl.h:401; NaN counts, as in the
    forward): they contribute nothing, and their grad_offset / grad_mask are exactly 0."""
    h, w = sample_coords(off, dg, K, stride, pad, dil)
    with np.errstate(invalid="ignore"):
        return ~((h > -1) & (w > -1) & (h < H) & (w < W))


def coord_offsets64(off, dg, K, stride, pad, dil):
    """float64 offsets that give the float64 oracle the kernels' own fp32 coordinate:
    off64 = float64(fl32(base + off)) - base.  Identity wherever base + off is exact in fp32;
    for the `margin` class's nextafter values next to a large base it is not, and the sample
    would otherwise sit on the other side of an integer (where grad_offset jumps)."""
    N, _, Ho, Wo = off.shape
    bh, bw = base_coords(K, Ho, Wo, stride, pad, dil)
    h, w = sample_coords(off, dg, K, stride, pad, dil)
    out = np.empty(off.shape, np.float64)
    o_h, o_w = split_offsets(out, dg, K)
    o_h[...] = h.reshape(N, dg, K, Ho, Wo).astype(np.float64) - bh[None, None]
    o_w[...] = w.reshape(N, dg, K, Ho, Wo).astype(np.float64) - bw[None, None]
    return out


def _edge_axis(rng, shape, size, base, counter, frac_mask, ulp):
    """Offsets of one axis for the edge / ulp classes: target - base with target cycling through
    {-1, 0, size-1, size} (`counter` picks it), or an odd multiple of 0.25 where frac_mask."""
    targets = np.array([-1, 0, size - 1, size])[counter % 4]
    o = (targets - base).astype(F32)  # integers: exact
    if ulp:
        direction = np.where(rng.integers(0, 2, shape) == 1, F32(np.inf), F32(-np.inf))
        o = np.nextafter(o, direction.astype(F32))
    frac = ((2 * rng.integers(-4, 4, shape) + 1) * 0.25).astype(F32)
    return np.where(frac_mask, frac, o).astype(F32), np.where(frac_mask, -99, targets)


def structured_offsets(rng, N, dg, K, Ho, Wo, H, W, stride, pad, dil, classes, with_targets=False):
    """-> (off float32 [N, dg*2*K, Ho, Wo], cls int8 [N, dg*K, Ho, Wo]): one class of `classes`
    (names of CLASSES) per sample, a seeded draw.

    zero    no offset
    int     integers in [-3, 3] on both axes
    half    multiples of 0.25 (so of 0.5 too) in [-3, 3]
    edge    off = target - base, target_h in {-1, 0, H-1, H}, target_w likewise: all 16
            combinations in turn (the four image corners among them), and mixed samples with one
            axis on an edge and the other fractional
    ulp     nextafter(target - base, +-inf) for the same targets
    margin  -2, nextafter(-2, -inf), nextafter(2, 0), 2, 2.5, -3 per axis (the other axis
            sometimes 0.5): inside the window forms' margin, the first value out, one corner out
    far     +-17, +-40, +-1e4, +-1e9, +-3e38, +-inf on h, on w, or on both
    nan     NaN on h, on w, or on both (forward tests only)

    with_targets: also return (target_h, target_w) int arrays [N, dg*K, Ho, Wo] for the edge / ulp
    samples (-99 elsewhere and on a fractional axis)."""
    ids = np.array([CID[c] for c in classes])
    shape = (N, dg, K, Ho, Wo)
    cls = ids[rng.integers(0, len(ids), shape)].astype(np.int8)
    bh, bw = base_coords(K, Ho, Wo, stride, pad, dil)
    bh = np.broadcast_to(bh[None, None], shape)
    bw = np.broadcast_to(bw[None, None], shape)
    oh, ow = np.zeros(shape, F32), np.zeros(shape, F32)
    th, tw = np.full(shape, -99), np.full(shape, -99)

    def put(name, vh, vw):
        sel = cls == CID[name]
        oh[sel], ow[sel] = vh[sel], vw[sel]
        return sel

    put("int", rng.integers(-3, 4, shape).astype(F32), rng.integers(-3, 4, shape).astype(F32))
    put("half", (rng.integers(-12, 13, shape) * 0.25).astype(F32),
        (rng.integers(-12, 13, shape) * 0.25).astype(F32))
    for name in ("edge", "ulp"):
        sel = cls == CID[name]
        # running index over the class's samples: the 16 target pairs come in turn
        counter = np.zeros(shape, np.int64)
        counter[sel] = np.arange(int(sel.sum()))
        variant = rng.integers(0, 4, shape)  # 0, 1: both axes on an edge; 2: w fractional; 3: h
        vh, t_h = _edge_axis(rng, shape, H, bh, counter // 4, variant == 3, name == "ulp")
        vw, t_w = _edge_axis(rng, shape, W, bw, counter, variant == 2, name == "ulp")
        put(name, vh, vw)
        th[sel], tw[sel] = t_h[sel], t_w[sel]
    mh = MARGIN_VALUES[rng.integers(0, len(MARGIN_VALUES), shape)]
    mw = MARGIN_VALUES[rng.integers(0, len(MARGIN_VALUES), shape)]
    mv = rng.integers(0, 4, shape)
    put("margin", np.where(mv == 3, F32(0.5), mh).astype(F32), np.where(mv == 2, F32(0.5), mw).astype(F32))
    for name, values in (("far", FAR_VALUES), ("nan", np.array([np.nan], F32))):
        fh = values[rng.integers(0, len(values), shape)]
        fw = values[rng.integers(0, len(values), shape)]
        near_h = rng.integers(-1, 2, shape).astype(F32)
        near_w = rng.integers(-1, 2, shape).astype(F32)
        axis = rng.integers(0, 3, shape)  # 0: h, 1: w, 2: both
        put(name, np.where(axis != 1, fh, near_h).astype(F32), np.where(axis != 0, fw, near_w).astype(F32))

    off = np.stack([oh, ow], 3).reshape(N, dg * 2 * K, Ho, Wo)
    cls = cls.reshape(N, dg * K, Ho, Wo)
    if with_targets:
        return off, cls, th.reshape(cls.shape), tw.reshape(cls.shape)
    return off, cls


def far_offsets_oracle(rng, off, cls, dg, K):
    """`off` with the far samples' values redrawn from FAR_VALUES_ORACLE (same axes, signs at
    random): the far class at sizes the CPU oracle can be called on."""
    off = off.copy()
    oh, ow = split_offsets(off, dg, K)
    sel = (cls == CID["far"]).reshape(oh.shape)
    for o in (oh, ow):
        big = sel & (np.abs(o) >= 17)
        o[big] = FAR_VALUES_ORACLE[rng.integers(0, len(FAR_VALUES_ORACLE), int(big.sum()))]
    return off


def sample_to_offset_mask(sel):
    """bool [N, dg*K, Ho, Wo] (per sample) -> bool [N, dg*2*K, Ho, Wo] (both offset components:
    channel g*2K + 2k + c belongs to sample g*K + k)."""
    N, SK, Ho, Wo = sel.shape
    return np.repeat(sel.reshape(N, SK, 1, Ho, Wo), 2, 2).reshape(N, 2 * SK, Ho, Wo)


def masked_equivalent(off, msk, sel):
    """The same problem with the selected samples (bool [N, dg*K, Ho, Wo]) switched off: their
    mask 0 and their offsets 0 -> (off0, msk0).  For samples that are invalid (outside the image
    or NaN), the forward output, grad_input, grad_weight and grad_bias of the original problem are
    this problem's, and its grad_mask / grad_offset are this problem's with the selected samples
    set to 0 (zero_selected): an invalid sample contributes val = 0 and mask-gradient 0, a
    masked-out one val * 0 and a mask-gradient nobody asks for."""
    assert off.shape[1] == 2 * sel.shape[1] and msk.shape == sel.shape
    off0 = np.where(sample_to_offset_mask(sel), 0, off).astype(off.dtype)
    msk0 = np.where(sel, 0, msk).astype(msk.dtype)
    return off0, msk0


def zero_selected(grad_offset, grad_mask, sel):
    """The masked problem's grad_offset / grad_mask with the selected samples set to 0."""
    return np.where(sample_to_offset_mask(sel), 0, grad_offset), np.where(sel, 0, grad_mask)


MASK_LOGITS = np.array([0, 20, -20, 88, -88, 100, -100, np.inf, -np.inf], F32)


def structured_logits(rng, shape):
    """Mask logits of the fused entries: the classes {0, +-20, +-88, +-100, +-inf} (expf over- and
    underflows, sigmoid exactly 0 and 1) for two samples in three, a standard normal draw else."""
    pick = rng.integers(0, len(MASK_LOGITS) + len(MASK_LOGITS) // 2, shape)
    lg = rng.standard_normal(shape).astype(F32)
    named = pick < len(MASK_LOGITS)
    lg[named] = MASK_LOGITS[pick[named]]
    return lg


def sigmoid_mask64(logits, mask_scale=2.0):
    """mask_scale * sigmoid(logits) in float64 (deform.py:86-89)."""
    with np.errstate(over="ignore"):
        return mask_scale / (1.0 + np.exp(-logits.astype(np.float64)))


# ---- the runs and shapes of tests/test_gpu_dcn_offsets.py (test_dcn_offsets_cpu.py checks that
# every class of every run is populated at every shape) -----------------------------------------
# One reference per run: the float64 oracle for exactly representable coordinates, the float32
# oracle for `ulp` (its coordinate is the same single fp32 add, so the validity decisions must
# agree), masked_equivalent (then the float64 oracle) for `far` and the forward's `nan`.
RUNS_BWD = {
    "exact": EXACT,
    "ulp": ("ulp", "zero", "int", "half", "edge"),
    "far": ("far", "zero", "int", "half", "edge", "margin"),
}
RUNS_FWD = dict(RUNS_BWD, far=RUNS_BWD["far"] + ("nan",))

# N, C, H, W, Co, k, stride, pad, dil, dg, groups
FWD_GENERIC = [
    (1, 64, 9, 20, 64, 3, 1, 2, 2, 2, 1),
    (1, 128, 16, 20, 128, 3, 2, 1, 1, 2, 1),
    (1, 24, 7, 11, 40, 3, 1, 1, 1, 3, 2),
]
FWD_WINDOW = [(1, c, h, w, c, 3, 1, 2, 2, 2, 1) for c, h, w in ((64, 13, 36), (32, 9, 28), (128, 13, 36))]
FWD_TILE = [(1, c, 13, 36, c, 3, 1, 2, 2, 2, 1) for c in (64, 32)]
FWD_SMALL = [(1, 16, 13, 37, 16, 3, 1, 2, 2, 2, 1), (1, 16, 3, 2, 16, 3, 1, 1, 1, 2, 1)]
# N, C, H, W, Co, k, stride, pad, dil, dg (groups 1)
BWD = [
    (1, 32, 9, 18, 32, 3, 1, 2, 2, 2),      # two ragged 8 x 8 tiles
    (1, 64, 10, 12, 64, 3, 1, 2, 2, 2),
    (1, 128, 16, 20, 128, 3, 2, 2, 2, 2),   # 64-channel groups: four slices, two weight-gradient
                                            # blocks, the stride-2 window
    (1, 48, 10, 21, 36, 3, 2, 1, 1, 3),     # global form only
]
MIN_PER_CLASS = 8


def out_hw(H, W, k, stride, pad, dil):
    f = lambda n: (n + 2 * pad - (dil * (k - 1) + 1)) // stride + 1  # noqa: E731
    return f(H), f(W)


def shape_offsets(shape, classes, seed=0, with_targets=False):
    """structured_offsets for one row of the shape tables (10 or 11 fields), seeded by the shape,
    the class set and `seed`."""
    N, C, H, W, Co, k, stride, pad, dil, dg = shape[:10]
    Ho, Wo = out_hw(H, W, k, stride, pad, dil)
    key = [seed, N, C, H, W, Co, k, stride, pad, dil, dg] + [CID[c] for c in classes]
    rng = np.random.default_rng(key)
    return structured_offsets(rng, N, dg, k * k, Ho, Wo, H, W, stride, pad, dil, classes,
                              with_targets=with_targets)


def class_counts(cls, classes):
    return {c: int((cls == CID[c]).sum()) for c in classes}


def window_sides(off, dg, K, H, W, stride, pad, dil, margin=2):
    """(inside, outside): valid samples whose offsets both lie in [-margin, margin) -- the window
    forms keep all four corners in the LDS window -- and valid samples with an offset outside it
    (a corner may leave the window: global atomic / global gather)."""
    oh, ow = (o.reshape(off.shape[0], dg * K, *off.shape[2:]) for o in split_offsets(off, dg, K))
    ok = ~invalid_samples(off, dg, K, H, W, stride, pad, dil)
    with np.errstate(invalid="ignore"):
        inner = (oh >= -margin) & (oh < margin) & (ow >= -margin) & (ow < margin)
    return int((ok & inner).sum()), int((ok & ~inner).sum())

"""CPU checks of the structured-offset helper (tests/dcn_offsets.py) that the GPU tests of
tests/test_gpu_dcn_offsets.py rest on: the masked-problem reference construction is pinned on the
CPU oracle, every class of every run is populated at every shape, and the edge offsets land on
their targets exactly."""
import numpy as np
import pytest

from oracle import oracle
from tests import dcn_offsets as do

ALL_FWD = do.FWD_GENERIC + do.FWD_WINDOW + do.FWD_TILE + do.FWD_SMALL
_ids = lambda s: "x".join(map(str, s))  # noqa: E731


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", [(1, 8, 7, 9, 8, 3, 1, 2, 2, 2), (2, 6, 6, 11, 4, 3, 2, 1, 1, 3)], ids=_ids)
def test_masked_equivalent_is_bit_equal_on_the_oracle(shape, dtype):
    """Far samples (+-17 ... +-1e6 on h, w or both -- sizes at which the oracle's (int)ih is still
    defined) that lie outside the image: the forward output and all five gradients of the problem
    equal, bit for bit, those of the problem with these samples' mask and offsets set to 0, with
    the samples' grad_offset / grad_mask exactly 0."""
    N, C, H, W, Co, k, s, p, d, dg = shape
    off, cls = do.shape_offsets(shape, do.RUNS_BWD["far"])
    rng = np.random.default_rng(3)
    off = do.far_offsets_oracle(rng, off, cls, dg, k * k)
    far = cls == do.CID["far"]
    sel = far & do.invalid_samples(off, dg, k * k, H, W, s, p, d)
    assert sel.sum() >= do.MIN_PER_CLASS and np.abs(off).max() == 1e6
    Ho, Wo = off.shape[2:]
    x = rng.standard_normal((N, C, H, W)).astype(np.float32)
    msk = rng.uniform(0, 2, cls.shape).astype(np.float32)
    w = (rng.standard_normal((Co, C, k, k)) / np.sqrt(C * k * k)).astype(np.float32)
    b = rng.standard_normal(Co).astype(np.float32)
    go = rng.standard_normal((N, Co, Ho, Wo)).astype(np.float32)
    off0, msk0 = do.masked_equivalent(off, msk, sel)
    assert np.array_equal(oracle.mdcn_forward(x, off, msk, w, b, s, p, d, 1, dg, dtype=dtype),
                          oracle.mdcn_forward(x, off0, msk0, w, b, s, p, d, 1, dg, dtype=dtype))
    got = oracle.mdcn_backward(x, off, msk, w, go, True, s, p, d, 1, dg, dtype=dtype)
    ref = oracle.mdcn_backward(x, off0, msk0, w, go, True, s, p, d, 1, dg, dtype=dtype)
    goff0, gm0 = do.zero_selected(ref[1], ref[2], sel)
    assert ref[2][sel].any()  # the masked problem's own grad_mask there is not 0
    for name, a, r in zip(("grad_input", "grad_offset", "grad_mask", "grad_weight", "grad_bias"), got,
                          (ref[0], goff0, gm0, ref[3], ref[4])):
        assert np.array_equal(a, r), name
    assert not got[1][do.sample_to_offset_mask(sel)].any() and not got[2][sel].any()


def _runs_and_shapes():
    for shape in ALL_FWD:
        for run, classes in do.RUNS_FWD.items():
            yield pytest.param(shape, classes, id=f"fwd-{_ids(shape)}-{run}")
    for shape in do.BWD:
        for run, classes in do.RUNS_BWD.items():
            yield pytest.param(shape, classes, id=f"bwd-{_ids(shape)}-{run}")


@pytest.mark.parametrize("shape,classes", _runs_and_shapes())
def test_structured_offsets_populate_every_class(shape, classes):
    """At least MIN_PER_CLASS samples of every requested class at every shape of the GPU tests,
    nothing of any other class; far values of 1e4 and beyond and NaNs are invalid samples, the
    16 edge target pairs (the four image corners among them) all occur."""
    N, C, H, W, Co, k, s, p, d, dg = shape[:10]
    off, cls, th, tw = do.shape_offsets(shape, classes, with_targets=True)
    Ho, Wo = do.out_hw(H, W, k, s, p, d)
    assert off.dtype == np.float32 and off.shape == (N, dg * 2 * k * k, Ho, Wo)
    assert cls.shape == (N, dg * k * k, Ho, Wo)
    counts = do.class_counts(cls, classes)
    assert min(counts.values()) >= do.MIN_PER_CLASS, counts
    assert sum(counts.values()) == cls.size
    inv = do.invalid_samples(off, dg, k * k, H, W, s, p, d)
    oh, ow = (o.reshape(cls.shape) for o in do.split_offsets(off, dg, k * k))
    with np.errstate(invalid="ignore"):
        big = ~((np.abs(oh) < 1e4) & (np.abs(ow) < 1e4))
    assert inv[big].all()
    for name in ("far", "nan"):
        if name in classes:
            assert big[cls == do.CID[name]].sum() >= do.MIN_PER_CLASS
    assert not big[~np.isin(cls, [do.CID["far"], do.CID["nan"]])].any()
    for name in ("edge", "ulp"):
        if name in classes and cls.size >= 1000:
            sel = (cls == do.CID[name]) & (th != -99) & (tw != -99)
            pairs = set(zip(th[sel].tolist(), tw[sel].tolist()))
            assert pairs == {(a, b) for a in (-1, 0, H - 1, H) for b in (-1, 0, W - 1, W)}


@pytest.mark.parametrize("shape", ALL_FWD + do.BWD, ids=_ids)
def test_edge_offsets_land_on_their_targets(shape):
    """fl32(base + off) == target for the edge class, on whichever axes carry a target; the ulp
    class lands within one ulp (of the offset) of the target, and both validity outcomes
    occur."""
    N, C, H, W, Co, k, s, p, d, dg = shape[:10]
    for name in ("edge", "ulp"):
        off, cls, th, tw = do.shape_offsets(shape, (name, "zero"), with_targets=True)
        h, w = do.sample_coords(off, dg, k * k, s, p, d)
        sel = cls == do.CID[name]
        oh, ow = (a.reshape(cls.shape) for a in do.split_offsets(off, dg, k * k))
        for coord, tgt, o in ((h, th, oh), (w, tw, ow)):
            on = sel & (tgt != -99)
            assert on.sum() >= do.MIN_PER_CLASS
            t = tgt[on].astype(np.float32)
            if name == "edge":
                assert np.array_equal(coord[on], t)
            else:
                # within one ulp of the larger of |off| and |target| (the add may round onto it)
                step = np.spacing(np.maximum(np.abs(o[on]), np.abs(t)).astype(np.float32))
                assert (np.abs(coord[on] - t) <= step).all()
                assert (coord[on] != t).sum() >= do.MIN_PER_CLASS // 2
        inv = do.invalid_samples(off, dg, k * k, H, W, s, p, d)[sel]
        assert inv.any() and not inv.all()

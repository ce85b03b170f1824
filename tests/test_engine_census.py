"""Coverage census of the conv engine's kernel instances (CPU only).

conv_fwd_kernel (aanet_amd/csrc/mdcn.hip) is one template with many instances, and launch_fwd
picks among them from the sizes at run time.  This census maps every case of the unit suites'
tables through ops.conv_engine_plan (the function launch_fwd itself launches from) to the key

    (mode, tail, prec, full, cfg, halo, layout, co_t, ptt)

and asserts that each key of REQUIRED is reached by at least one case whose last tile is ragged
(the guards of a tile that is not full are what a kernel instance gets wrong on its own).  A key
the tables reach that is in neither REQUIRED nor NOT_REQUIRED fails: a new instance, or a new
route to an old one, has to be classified here.  Cases that an entry point diverts to a
specialised kernel before the engine (direct few-channel conv, streaming 1x1, window / 16-channel
DCN; include/aanet_mi355x.h, aanet_conv_engine_plan) never run the engine and are not counted.
"""
import collections

from aanet_amd import _lib, ops
from tests import test_gpu_conv as tc
from tests import test_gpu_engine_tiles as tt
from tests import test_gpu_split as ts

SPLIT, EXACT, GENERIC = _lib.CONV_WEIGHTS_SPLIT, _lib.CONV_EXACT_F32, _lib.CONV_GENERIC_DCN
KEY = "mode tail prec full cfg halo layout co_t ptt".split()


def has_split_pack(Co, Cg, k, g):
    return _lib.lib().aanet_conv_weight_pack_split_bytes(Co, Cg, k, k, g) > 0


def diverted_plain(N, C, H, W, Co, k, s, p, d, g, layout, split):
    """aanet_conv2d_fused_f32's dispatch before the engine, as include/aanet_mi355x.h lists it."""
    if layout in (0, 1) and g == 1 and d == 1:  # direct few-channel kernel
        nchw = layout == 0
        if nchw and ((C, k, s) == (3, 7, 3) and Co <= 32 or (C, k, s) == (3, 3, 1) and Co <= 32
                     or (C, k, s) in ((6, 3, 1), (1, 3, 1)) and Co <= 16):
            return "direct"
        if (C, k, s, Co) == (32, 3, 1, 1):
            return "direct"
    if split and (k, s, p, g) == (1, 1, 0, 1) and C in (32, 64) and \
            (Co <= 64 or (Co <= 512 and Co % 64 == 0 and not layout & 1)) and (not layout & 2 or Co % 4 == 0):
        return "pointwise"
    return None


def census():
    """-> {key: [(case name, ragged)]} over every table, and the diverted case names."""
    seen, diverted = collections.defaultdict(list), []

    def add(name, mode, pl):
        assert pl.status == 0, (name, pl)
        key = (mode, pl.tail, pl.prec, pl.full, pl.cfg, pl.halo, pl.layout, pl.co_t, pl.ptt)
        seen[key].append((name, pl.last_tile_pixels != 0))

    def plain(name, case, layout, weights, exact=False):
        N, C, H, W, Co, k, s, p, d, g = case
        split = weights == "split" and not exact
        why = diverted_plain(N, C, H, W, Co, k, s, p, d, g, layout, split)
        if why:
            diverted.append((name, why))
            return
        add(name, 0, ops.conv_engine_plan("conv", N, C, H, W, Co, k, s, p, d, g,
                                          layout=layout | tt.flags_of(weights, exact),
                                          packed=weights != "raw"))

    # tests/test_gpu_conv.py
    for i, case in enumerate(tc.CONV_CASES):
        N, C, H, W, Co, k, s, p, d, g = case
        for packed in (False, True, "split"):
            weights = {False: "raw", True: "packed"}.get(packed, "split")
            if weights == "split" and not has_split_pack(Co, C // g, k, g):
                weights = "packed"  # test_gpu_conv._packed falls back to pack_weight
            plain(f"conv.CONV_CASES[{i}]/{packed}", case, 0, weights)
    for i, case in enumerate(tc.NHWC_CASES):
        for layout in (1, 2, 3):
            if layout & 2 and (case[4] // case[9]) % 4:
                continue  # skipped there too: NHWC output needs (Co / groups) % 4 == 0
            plain(f"conv.NHWC_CASES[{i}]/layout{layout}", case, layout, "packed")
    for i, (N, C, H, W, Co, d) in enumerate(tc.PHASE_CASES):
        plain(f"conv.PHASE_CASES[{i}]", (N, C, H, W, Co, 3, 1, d, d, 1), 3, "split")
    for table, nhwc in ((tc.PW_TAIL_CASES, 0), (tc.PW_TAIL_NHWC_CASES, 1)):
        for C, H, W in table:
            add(f"conv.pw_tail[{C},{H},{W}]/nhwc{nhwc}", 0,
                ops.conv_engine_plan("conv", 2, C, H, W, C, 3, 1, 1, 1, co2=C, layout=nhwc))
    for C, H, W in tc.MDCN_TAIL_CASES:
        if C == 16:
            diverted.append((f"conv.mdcn_tail[{C}]", "dcn_small"))
            continue
        add(f"conv.mdcn_tail[{C},{H},{W}]", 1,
            ops.conv_engine_plan("dcn", 2, C, H, W, C, 3, 1, 2, 2, 1, 2, co2=C))
    for C, H, W, _, dg in tc.MDCN_TAIL_NHWC_CASES:  # plain packs: no window kernel
        for nhwc in (1, 0):
            add(f"conv.mdcn_tail_nhwc[{C},{H},{W},dg{dg}]/nhwc{nhwc}", 1,
                ops.conv_engine_plan("dcn", 2, C, H, W, C, 3, 1, 2, 2, 1, dg, co2=C, layout=nhwc))
    # tests/test_gpu_split.py: every case runs the split and the exact contraction
    for i, case in enumerate(ts.SPLIT_CASES):
        for exact in (False, True):
            plain(f"split.SPLIT_CASES[{i}]/{'exact' if exact else 'split'}", case[:10], int(case[10]),
                  "split", exact)
    # tests/test_gpu_engine_tiles.py
    for case in tt.PLAIN_CASES + tt.LAYOUT_CASES:
        name, N, C, (H, W), Co, k, s, p, d, g, weights, exact, layout, _ = case
        assert diverted_plain(N, C, H, W, Co, k, s, p, d, g, layout, weights == "split" and not exact) is None, name
        add("tiles." + name, 0, tt.plain_plan(case))
    for case in tt.TAIL_CASES:
        add("tiles." + case[0], 0, tt.tail_plan(case))
    for case in tt.DCN_CASES:
        add("tiles." + case[0], 1, tt.dcn_plan(case))
    return seen, diverted


# Every ptt = 128 key of tests/test_gpu_engine_tiles.py, the halo keys, and the ptt = 64 keys the
# older suites cover: each needs a case with a ragged last tile.
#   mode tail prec full cfg halo layout co_t ptt
REQUIRED = [
    (0, 0, 0, 0, 0, 0, 0, 32, 64),    # 5x5 stride-2 stem from the image (tests/stage_sweep.py)
    (0, 0, 0, 0, 0, 0, 0, 16, 128),
    (0, 0, 0, 0, 0, 0, 0, 64, 128),
    (0, 0, 0, 1, 0, 0, 0, 32, 64),
    (0, 0, 0, 1, 0, 0, 0, 32, 128),
    (0, 0, 0, 1, 0, 0, 0, 64, 64),
    (0, 0, 0, 1, 0, 0, 0, 64, 128),
    (0, 0, 0, 1, 0, 0, 1, 16, 128),
    (0, 0, 0, 1, 0, 0, 1, 32, 64),
    (0, 0, 0, 1, 0, 0, 1, 64, 64),
    (0, 0, 0, 1, 0, 0, 1, 64, 128),
    (0, 0, 0, 1, 0, 0, 2, 32, 64),
    (0, 0, 0, 1, 0, 0, 2, 32, 128),
    (0, 0, 0, 1, 0, 0, 2, 64, 64),
    (0, 0, 0, 1, 0, 0, 3, 32, 64),
    (0, 0, 0, 1, 0, 0, 3, 64, 64),
    (0, 0, 0, 1, 0, 0, 3, 64, 128),
    (0, 0, 0, 1, 1, 0, 0, 32, 128),
    (0, 0, 0, 1, 1, 0, 0, 64, 128),
    (0, 0, 0, 1, 1, 0, 1, 32, 128),
    (0, 0, 0, 1, 1, 0, 2, 32, 128),
    (0, 0, 0, 1, 1, 0, 3, 32, 128),
    (0, 0, 1, 0, 0, 0, 0, 32, 128),
    (0, 0, 1, 0, 0, 0, 0, 64, 128),
    (0, 0, 1, 1, 0, 0, 0, 32, 64),
    (0, 0, 1, 1, 0, 0, 0, 32, 128),
    (0, 0, 1, 1, 0, 0, 0, 64, 64),
    (0, 0, 1, 1, 0, 0, 0, 64, 128),
    (0, 0, 1, 1, 0, 0, 1, 64, 128),
    (0, 0, 1, 1, 0, 0, 2, 32, 128),
    (0, 0, 1, 1, 0, 0, 3, 32, 128),
    (0, 0, 1, 1, 0, 0, 3, 64, 128),
    (0, 0, 1, 1, 0, 1, 1, 32, 128),
    (0, 0, 1, 1, 0, 1, 1, 64, 128),
    (0, 0, 1, 1, 0, 2, 1, 32, 128),
    (0, 0, 1, 1, 0, 2, 1, 64, 128),
    (0, 0, 1, 1, 0, 1, 3, 32, 128),   # _DilatedStack's dilation-1 / 2 convs, NHWC in and out
    (0, 0, 1, 1, 0, 2, 3, 32, 128),
    (0, 0, 1, 1, 0, 4, 3, 32, 128),
    (0, 0, 1, 1, 0, 4, 3, 64, 128),
    (0, 1, 0, 0, 0, 0, 0, 16, 128),
    (0, 1, 0, 1, 0, 0, 0, 32, 64),
    (0, 1, 0, 1, 0, 0, 0, 64, 64),
    (0, 1, 0, 1, 0, 0, 0, 64, 128),
    (0, 1, 0, 1, 0, 0, 1, 64, 64),
    (0, 1, 0, 1, 0, 0, 1, 64, 128),
    (0, 1, 0, 1, 1, 0, 0, 64, 128),
    (0, 1, 1, 1, 0, 0, 0, 32, 128),
    (0, 1, 1, 1, 0, 0, 0, 64, 128),
    (0, 1, 1, 1, 0, 0, 1, 64, 128),
    (1, 0, 0, 1, 0, 0, 0, 64, 128),
    (1, 0, 0, 1, 0, 0, 1, 64, 128),
    (1, 0, 0, 1, 2, 0, 0, 32, 128),
    (1, 0, 0, 1, 2, 0, 1, 32, 128),
    (1, 0, 1, 1, 0, 0, 0, 64, 128),
    (1, 0, 1, 1, 0, 0, 1, 64, 128),
    (1, 1, 0, 1, 0, 0, 0, 32, 64),
    (1, 1, 0, 1, 0, 0, 0, 64, 64),
    (1, 1, 0, 1, 0, 0, 0, 64, 128),
    (1, 1, 0, 1, 0, 0, 1, 32, 64),
    (1, 1, 0, 1, 0, 0, 1, 64, 64),
    (1, 1, 0, 1, 2, 0, 0, 32, 64),
    (1, 1, 0, 1, 2, 0, 0, 64, 64),
    (1, 1, 0, 1, 2, 0, 1, 32, 64),
    (1, 1, 0, 1, 2, 0, 1, 64, 64),
    (1, 1, 1, 1, 0, 0, 0, 64, 128),
    (1, 1, 1, 1, 0, 0, 1, 64, 128),
]

# Keys the tables reach (or launch_fwd_f can launch) that the census does not hold to a ragged case.
NOT_REQUIRED = {
    # halo-tile tails (3x3 stride 1 on NHWC input + pointwise tail, with or without the post stage)
    **{(0, 1, 1, 1, 0, h, 1, c, 128): "halo-tile tail: no fp64 table yet; held to the exact engine in "
       "test_split_tail_kernels_match_exact and to the reference in the production / model suites"
       for h in (1, 2) for c in (32, 64)},
    # split contraction on 64-pixel tiles with an NHWC side (no halo form: stride 2, 1x1 past the
    # pointwise kernel, NCHW input)
    **{(0, 0, 1, 1, 0, 0, lay, c, 64): "single-shape tests outside the tables "
       "(test_stride2_nhwc_output_vs_torch); the 128-pixel sibling is required"
       for lay in (1, 2, 3) for c in (32, 64)},
    **{(0, 1, 1, 1, 0, 0, lay, c, 64): "split tails on 64-pixel tiles: small NHWC shapes take the halo "
       "form, NCHW ones run in the model suites; the 128-pixel sibling is required"
       for lay in (0, 1) for c in (32, 64)},
    # the op-level deformable conv below the threshold: tests/test_gpu_mdcn.py (its own tables,
    # against the oracle bit for bit on the sampler) and test_split_dcn_accuracy_vs_fp64_oracle
    **{(1, 0, prec, full, cfg, 0, lay, c, 64): "op-level DCN on 64-pixel tiles: tests/test_gpu_mdcn.py"
       for prec in (0, 1) for full in (0, 1) for cfg in (0, 2) for lay in (0, 1) for c in (32, 64)},
    **{(1, tail, 0, 0, 0, 0, 0, c, 128): "guarded DCN chunks (C / dg not a multiple of 16) or 16-channel "
       "tiles: tests/test_gpu_mdcn.py" for tail in (0, 1) for c in (16, 32, 64)},
    **{(1, 1, 1, 1, 0, 0, lay, 64, 64): "split DCN tail on 64-pixel tiles: test_split_tail_kernels_match_exact; "
       "the 128-pixel sibling is required" for lay in (0, 1)},
    # 128-pixel keys outside section 3 of the plan this census was written for
    **{(1, 1, 0, 1, 2, 0, lay, c, 128): "CFG 2 DCN tail at 128-pixel tiles: CFG 2 is required through the "
       "op-level forms, the tail through CFG 0" for lay in (0, 1) for c in (32, 64)},
    **{(1, 0, 0, 1, 0, 0, lay, 32, 128): "DCN with <= 32 outputs and 32-channel deformable groups at "
       "128-pixel tiles: no caller (C = Co in every AANet DCN)" for lay in (0, 1)},
    **{(0, 1, prec, 1, cfg, 0, lay, 32, 128): "32-channel plain tails in exact f32 / 16-channel chunks "
       "at 128-pixel tiles: the split NCHW one is required" for prec in (0, 1) for cfg in (0, 1)
       for lay in (0, 1) if (prec, cfg, lay) != (1, 0, 0)},
    **{(0, 0, 0, 1, 1, 0, lay, 64, 128): "16-channel chunks with a 64-channel tile and an NHWC side: "
       "the 32-channel tile's three layouts are required" for lay in (1, 2, 3)},
}


def test_engine_instance_census():
    seen, diverted = census()
    print("\nmode tail prec full cfg halo layout co_t ptt | cases ragged")
    for key in sorted(seen):
        cases = seen[key]
        print(" ".join(f"{v:>{len(h)}}" for h, v in zip(KEY, key)), "|",
              f"{len(cases):5d} {sum(r for _, r in cases):6d}",
              "" if key in REQUIRED else "  (not required)")
    print(f"{len(seen)} keys, {sum(map(len, seen.values()))} engine cases; diverted before the engine: "
          f"{collections.Counter(w for _, w in diverted).most_common()}")
    assert len(set(REQUIRED)) == len(REQUIRED) and not set(REQUIRED) & set(NOT_REQUIRED)
    unclassified = sorted(set(seen) - set(REQUIRED) - set(NOT_REQUIRED))
    assert not unclassified, f"keys in neither REQUIRED nor NOT_REQUIRED: {unclassified}"
    for key in REQUIRED:
        ragged = [n for n, r in seen.get(key, []) if r]
        assert ragged, f"{dict(zip(KEY, key))}: no case with a ragged last tile " \
                       f"({[n for n, _ in seen.get(key, [])] or 'no case at all'})"


def test_engine_tiles_cases_cover_every_128_pixel_key_they_name():
    """Each case of tests/test_gpu_engine_tiles.py lands on a required ptt = 128, halo 0 key with
    a ragged last tile (what the GPU test asserts before it runs, here without a GPU)."""
    for case, plan, mode in ([(c, tt.plain_plan, 0) for c in tt.PLAIN_CASES + tt.LAYOUT_CASES]
                             + [(c, tt.tail_plan, 0) for c in tt.TAIL_CASES]
                             + [(c, tt.dcn_plan, 1) for c in tt.DCN_CASES]):
        pl = plan(case)
        assert pl.status == 0 and pl.ptt == 128 and pl.halo == 0 and 0 < pl.last_tile_pixels < 128, case[0]
        assert {k: getattr(pl, k) for k in case[-1]} == case[-1], (case[0], pl)
        assert (mode, pl.tail, pl.prec, pl.full, pl.cfg, 0, pl.layout, pl.co_t, 128) in REQUIRED, case[0]

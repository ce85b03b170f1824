"""Loading helpers for the committed golden fixtures (data only, no pickles)."""
import functools
import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden_names(prefix):
    return sorted(f[:-4] for f in os.listdir(GOLDEN_DIR) if f.startswith(prefix) and f.endswith(".npz"))


@functools.lru_cache(maxsize=None)
def golden(name):
    with np.load(os.path.join(GOLDEN_DIR, name + ".npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def state_dict_of(g):
    """Fixture keys 'param.<name>' -> {name: array} (reference state-dict keys)."""
    return {k[len("param."):]: v for k, v in g.items() if k.startswith("param.")}


def synthetic_value(name, shape, seed):
    """Deterministic value of one state-dict entry, keyed by its name (torch CPU generator).
    Shared by tests/golden/make_model_golden.py (filling the REFERENCE model) and the tests
    (filling ours): equal names + shapes => equal tensors, so the full-model fixtures need not
    carry megabytes of weights, and a name mismatch is a checkpoint-compatibility failure."""
    import zlib

    import torch
    g = torch.Generator().manual_seed((zlib.crc32(name.encode()) * 1000003 + seed) % (1 << 62))
    leaf = name.rsplit(".", 1)[-1]
    shape = tuple(shape)
    if leaf == "num_batches_tracked":
        return torch.zeros(shape, dtype=torch.long)
    if leaf == "running_mean":
        return 0.1 * torch.randn(shape, generator=g)
    if leaf == "running_var":
        return 0.5 + torch.rand(shape, generator=g)
    if leaf == "bias":
        return (0.5 if "offset_conv" in name else 0.1) * torch.randn(shape, generator=g)
    if len(shape) == 1:  # norm-layer gamma
        return 1.0 + 0.1 * torch.randn(shape, generator=g)
    fan_in = 1
    for s in shape[1:]:
        fan_in *= s
    return (2 * torch.rand(shape, generator=g) - 1) * (3.0 / fan_in) ** 0.5


def fill_synthetic(module, seed, scales=None):
    """Overwrite every parameter and buffer of `module` with synthetic_value; returns the
    (name, shape) list in state-dict order.  `scales` ({state-dict name: factor}, a fixture's
    `scales` entry) multiplies named entries after the fill: the conditioning of a fixture whose
    plain fill drives the network into a near-tie regime (make_model_golden.py, psmnet_aa)."""
    import torch
    sd = module.state_dict()
    scales = dict(scales or {})
    with torch.no_grad():
        for k, v in sd.items():
            v.copy_(synthetic_value(k, v.shape, seed).to(v.dtype))
            if k in scales:
                v.mul_(float(scales.pop(k)))
    assert not scales, f"scaled names not in the model: {sorted(scales)}"
    return [(k, tuple(v.shape)) for k, v in sd.items()]


def fixture_scales(g):
    """The conditioning scales a model fixture was generated with ({} when none)."""
    import json
    return json.loads(str(g["scales"])) if "scales" in g else {}


def synthetic_pair(B, H, W, seed):
    """Seeded synthetic stereo pair for the full-model fixtures (torch CPU generator): right =
    left shifted 6 px left + noise, so the matching has a real answer."""
    import torch
    gm = torch.Generator().manual_seed(1000 + seed)
    left = torch.rand(B, 3, H, W, generator=gm) * 2 - 1
    right = torch.roll(left, shifts=-6, dims=3) + 0.05 * torch.randn(B, 3, H, W, generator=gm)
    return left, right


def synthetic_pyramid(B, C, H, W, seed, num_scales=3, channels=None):
    """Seeded N(0,1) feature pyramids (left, right) at H>>s x W>>s, s < num_scales (torch CPU
    generator), for the production-configuration fixtures: the test rebuilds them from the seed,
    so the fixture carries outputs only.  `channels` gives per-scale widths (AANet+'s
    FeaturePyrmaid: 32/64/128, nets/feature.py:379-419); otherwise every scale has C."""
    import torch
    g = torch.Generator().manual_seed(5000 + seed)
    cs = list(channels) if channels is not None else [C] * num_scales
    left = [torch.randn(B, cs[s], H >> s, W >> s, generator=g) for s in range(num_scales)]
    right = [torch.randn(B, cs[s], H >> s, W >> s, generator=g) for s in range(num_scales)]
    return left, right


def synthetic_pyramid_sizes(B, C, sizes, seed):
    """synthetic_pyramid with explicit per-scale (H, W) `sizes` (a pyramid whose coarse scales
    are ceil- or floor-halved, or one row high): seeded N(0,1) (left, right) lists of
    [B, C, H_s, W_s] tensors.  Its own generator stream (seed base 7000): no fixture depends on
    it, and synthetic_pyramid's draws are untouched."""
    import torch
    g = torch.Generator().manual_seed(7000 + seed)
    left = [torch.randn(B, C, h, w, generator=g) for h, w in sizes]
    right = [torch.randn(B, C, h, w, generator=g) for h, w in sizes]
    return left, right


def production_case(tag):
    """(fixture, numpy state dict of `aggregation.*` without the prefix, left pyramid, right
    pyramid) of a make_production_golden.py fixture: the weights are rebuilt by name on our own
    module tree (so a key mismatch with the reference fails here) and the inputs from the seed."""
    import torch

    from aanet_amd.nets import AANetHotPath
    g = golden(tag)
    B, C, H, W = (int(v) for v in g["shape"])
    seed, max_disp = int(g["seed"]), int(g["max_disp"])
    m = AANetHotPath(max_disp, no_intermediate_supervision=True, num_deform_blocks=3)
    names = fill_synthetic(m.aggregation, seed)
    assert [n for n, _ in names] == list(g["names"]), "state-dict keys differ from the reference"
    sd = {k: v.numpy() for k, v in m.aggregation.state_dict().items()}
    checksum = sum(float(torch.from_numpy(v).double().abs().sum()) for v in sd.values())
    assert abs(checksum - float(g["checksum"])) <= 1e-9 * abs(checksum), "weight fill differs"
    channels = [int(c) for c in g["channels"]] if "channels" in g else None
    left, right = synthetic_pyramid(B, C, H, W, seed, channels=channels)
    feat = sum(float(t.double().abs().sum()) for t in left + right)
    assert abs(feat - float(g["feat_checksum"])) <= 1e-9 * abs(feat), "feature fill differs"
    return g, sd, m, left, right

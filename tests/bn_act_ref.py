"""Float64 restatement of the fused training BatchNorm (aanet_amd/csrc/bn_act.hip), the reference
of tests/test_gpu_bn_act*.py (a helper module, not a test):

    y = act(gamma * (x - mean) * invstd + beta [+ residual])

with the batch mean and biased variance per channel over [N, S...], invstd = 1 / sqrt(var + eps).
The backward takes the activation's derivative from an OUTPUT, `y_mask` -- y > 0 -> 1, else 0
(relu) or 0.2 (leaky) --, which the GPU tests set to the device's own y: an fp32-vs-fp64 sign flip
of a near-zero output is not an error of the backward.

Also the error bars of the issue's test plan, from the number formats (u = 2^-24, K = 8).
"""
import torch

U = 2.0 ** -24
K = 8.0
TINY = 1e-30
ACTS = (None, "relu", "leaky")


def _per_channel(t, x):
    return t.to(torch.float64).view(1, -1, *([1] * (x.dim() - 2)))


def _dims(x):
    return [0] + list(range(2, x.dim()))


def act64(v, act):
    if act == "relu":
        return torch.where(v > 0, v, torch.zeros_like(v))
    if act == "leaky":
        return torch.where(v > 0, v, 0.2 * v)
    assert act is None
    return v


def forward(x, weight, bias, eps, act=None, residual=None):
    """-> dict: y, mean [C], var [C] (biased), invstd [C], xhat, count; everything float64."""
    x = x.to(torch.float64)
    dims = _dims(x)
    count = x.numel() // x.shape[1]
    mean = x.mean(dims)
    var = ((x - _per_channel(mean, x)) ** 2).mean(dims)
    invstd = 1.0 / torch.sqrt(var + eps)
    xhat = (x - _per_channel(mean, x)) * _per_channel(invstd, x)
    v = _per_channel(weight, x) * xhat + _per_channel(bias, x)
    if residual is not None:
        v = v + residual.to(torch.float64)
    return dict(y=act64(v, act), mean=mean, var=var, invstd=invstd, xhat=xhat, count=count)


def running(running_mean, running_var, mean, var, count, momentum):
    """The running-statistics update: (1 - m) * running + m * stat, variance unbiased."""
    rm = (1 - momentum) * running_mean.to(torch.float64) + momentum * mean
    rv = (1 - momentum) * running_var.to(torch.float64) + momentum * var * (count / (count - 1))
    return rm, rv


def act_grad(grad_out, y_mask, act):
    """g = grad_out * act'(y) with act' from an output: y > 0 -> 1, else 0 / 0.2."""
    g = grad_out.to(torch.float64)
    if act is None:
        return g
    neg = 0.0 if act == "relu" else 0.2
    return torch.where(y_mask.to(torch.float64) > 0, g, neg * g)


def backward(grad_out, x, weight, fwd, act=None, y_mask=None, with_residual=False):
    """-> dict: dx, dweight [C], dbias [C], dres (g, or None), g; fwd: forward()'s dict."""
    x = x.to(torch.float64)
    dims = _dims(x)
    g = act_grad(grad_out, y_mask, act)
    xhat = fwd["xhat"]
    sg, sgx = g.sum(dims), (g * xhat).sum(dims)
    n = fwd["count"]
    dx = _per_channel(weight.to(torch.float64) * fwd["invstd"], x) * (
        g - _per_channel(sg / n, x) - xhat * _per_channel(sgx / n, x))
    return dict(dx=dx, dweight=sgx, dbias=sg, dres=g if with_residual else None, g=g)


# ------------------------------------------------------------------------ error bars ---
def kappa(fwd):
    return 1.0 + fwd["mean"].abs() * fwd["invstd"]


def y_bar(x, weight, bias, fwd, residual=None):
    """|y - y64| <= K u (|gamma| (kappa + |xhat|) + |beta| + |residual|), per element."""
    b = _per_channel(weight.abs(), x) * (_per_channel(kappa(fwd), x) + fwd["xhat"].abs()) \
        + _per_channel(bias.abs(), x)
    if residual is not None:
        b = b + residual.to(torch.float64).abs()
    return K * U * b


def dx_bar(x, weight, fwd, g):
    """|dx - dx64| <= K u |gamma| invstd kappa max|g| max(1, max|xhat|), per channel."""
    dims = _dims(x)
    b = weight.to(torch.float64).abs() * fwd["invstd"] * kappa(fwd) * g.abs().amax(dims) \
        * fwd["xhat"].abs().amax(dims).clamp_min(1.0)
    return K * U * _per_channel(b, x)


def dweight_bar(x, fwd, g, dweight64):
    return K * U * (kappa(fwd) * g.abs().sum(_dims(x)) + dweight64.abs())


def dbias_bar(x, g):
    return K * U * g.abs().sum(_dims(x))


def rel_bar(ref):
    """K u relative (plus a denormal-sized floor for an exact zero)."""
    return K * U * ref.abs() + TINY

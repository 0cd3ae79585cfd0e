"""numpy restatement of the optimiser seam's host-visible arithmetic (include/drp.h: drp_train_accumulate, drp_train_apply), in
float64: the accumulator, the scaled global norm, torch's clip_grad_norm_ factor and the float32 gradient the Adam step is taken
on.  tests/test_optim_host.py holds it against torch.nn.utils.clip_grad_norm_; tests/test_gpu_optim.py holds the device to it."""
import numpy as np

CLIP_EPS = 1e-6     # torch.nn.utils.clip_grad_norm_: clip_coef = max_norm / (total_norm + 1e-6)


def accumulate(acc, grad, weight):
    """acc + weight * (double)grad, one rounding per addition; acc None: a zeroed accumulator"""
    grad = np.asarray(grad)
    acc = np.zeros(grad.shape, np.float64) if acc is None else np.asarray(acc, np.float64)
    return acc + np.float64(weight) * grad.astype(np.float64)


def norm(acc, scale):
    """|| scale * acc ||_2"""
    x = np.float64(scale) * np.asarray(acc, np.float64)
    return float(np.sqrt(np.sum(x * x)))


def clip(total_norm, max_norm=None):
    """min(1, max_norm / (total_norm + 1e-6)); None: no clipping"""
    if max_norm is None:
        return 1.0
    return float(min(1.0, np.float64(max_norm) / (np.float64(total_norm) + CLIP_EPS)))


def scaled_gradient(acc, scale, clip_coef=1.0):
    """(float)(acc * (scale * clip)): the gradient drp_train_apply steps on"""
    s = np.float64(scale) * np.float64(clip_coef)
    return (np.asarray(acc, np.float64) * s).astype(np.float32)


def apply(acc, scale, max_norm=None):
    """-> (norm, clip, the float32 gradient)"""
    n = norm(acc, scale)
    c = clip(n, max_norm)
    return n, c, scaled_gradient(acc, scale, c)

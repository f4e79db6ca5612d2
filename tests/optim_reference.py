"""Plain references for the optimiser / bookkeeping kernels of ga-ddpg_amd/csrc/optim.hip (include/gaddpg.h sections E-G) and
the two BatchNorm bookkeeping entry points.  numpy only (importable without a GPU), one element at a time in the obvious way,
written from torch.optim.Adam (L2 decay folded into the gradient, amsgrad=False), torch.nn.utils.clip_grad_norm_
(coef = min(1, max / (norm + 1e-6)), .grad scaled in place) and the reference project's soft_update / half_soft_update /
half_hard_update / module_max_param / module_max_gradient (core/utils.py).

Every function takes `dtype`: np.float64 is the reference, np.float32 the yardstick "r32" (what a careful float32
implementation of the same formulas gives).  Hyper-parameters enter as Python doubles -- betas = (0.9, 0.999), not their
float32 roundings -- and every derived scalar (1 - beta, lr / (1 - beta1**t), sqrt(1 - beta2**t), 1 - tau) is formed in
double and rounded to `dtype` once, which is what torch does with the Python scalars of its optimisers."""
import math

import numpy as np

BETAS = (0.9, 0.999)


def f32(x):
    """float64 -> float32, round to nearest even (numpy's conversion; pinned by tests/test_optim_reference.py)"""
    with np.errstate(over="ignore"):
        return np.asarray(x, dtype=np.float64).astype(np.float32)


# ----------------------------------------------------------------------------- gradient arena, sums of squares
def grad_from_arena(gacc, m2p, grad=None, accumulate=False):
    """grad[i] = float32(gacc[m2p[i]]) (m2p[i] < 0: 0); accumulate: added in float32 to the existing grad"""
    m2p = np.asarray(m2p)
    g = np.where(m2p >= 0, f32(np.asarray(gacc, np.float64)[np.maximum(m2p, 0)]), np.float32(0))
    g = g.astype(np.float32)
    if accumulate:
        with np.errstate(over="ignore", invalid="ignore"):
            g = (np.asarray(grad, np.float32) + g).astype(np.float32)
    return g


def sumsq_exact(g):
    """sum of the float64 squares of float32 values, correctly rounded (math.fsum; a float32 square is exact in float64)"""
    g = np.asarray(g, np.float32).astype(np.float64)
    return math.fsum((g * g).tolist())


def sumsq_bound(n, exact):
    """|kernel - exact| for a sum of n exact non-negative float64 terms added in ANY order with round-to-nearest adds:
    each of the n - 1 adds (n with the add into *out) commits at most 2**-53 of its own result, every partial result is at
    most the (computed) total, so the error is at most n * 2**-53 * total * (1 + O(n 2**-53)) <= n * 2**-52 * exact."""
    return n * 2.0 ** -52 * exact


# ----------------------------------------------------------------------------- clip_grad_norm_ + Adam
def clip_coef(sumsq, clip_max, dtype):
    """min(1, clip_max / (norm + 1e-6)) with the norm = sqrt(sumsq) rounded to dtype (torch holds it as a tensor of the
    gradients' dtype); sumsq is the float64 sum of squares.  None: no clipping."""
    if clip_max is None:
        return None
    dt = np.dtype(dtype).type
    with np.errstate(divide="ignore"):
        c = dt(clip_max) / (dt(math.sqrt(sumsq)) + dt(1e-6))
    return c if c < dt(1.0) else dt(1.0)


def adam_step(p, grad, m, v, hp, t, dtype, active=None, sumsq=None, clip_max=None, grad_scale=1.0):
    """One torch.optim.Adam step (single-tensor form, amsgrad=False, maximize=False) after clip_grad_norm_, over flat
    arrays.  hp: dict lr / betas / eps / weight_decay (Python doubles); t: the step number (>= 1).
    grad_scale multiplies the gradient together with the clip coefficient (include/gaddpg.h: `hyper[7]`).
    active[i] == 0: a parameter whose .grad is None -- nothing of it changes.
    -> (p, grad, exp_avg, exp_avg_sq) after the step; grad is the in-place scaled .grad (unchanged without a clip)."""
    dt = np.dtype(dtype).type
    p, g0, m, v = (np.asarray(x, np.float64).astype(dtype) for x in (p, grad, m, v))
    b1, b2 = hp["betas"]
    lr, eps, wd = hp["lr"], hp["eps"], hp["weight_decay"]
    act = np.ones(p.shape, bool) if active is None else np.asarray(active).astype(bool)
    coef = dt(grad_scale)
    c = clip_coef(sumsq, clip_max, dtype) if clip_max is not None else None
    if c is not None:
        coef = coef * c
    g = g0 * coef
    gw = g + dt(wd) * p if wd != 0 else g                         # grad.add(param, alpha=weight_decay)
    m1 = m + (gw - m) * dt(1.0 - b1)                              # exp_avg.lerp_(grad, 1 - beta1)
    v1 = v * dt(b2) + dt(1.0 - b2) * gw * gw                      # exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    step_size = lr / (1.0 - b1 ** t)
    bc2_sqrt = math.sqrt(1.0 - b2 ** t)
    denom = np.sqrt(v1) / dt(bc2_sqrt) + dt(eps)
    p1 = p - dt(step_size) * (m1 / denom)                         # param.addcdiv_(exp_avg, denom, value=-step_size)
    out_g = np.where(act, g, g0) if c is not None else g0
    return (np.where(act, p1, p).astype(dtype), out_g.astype(dtype), np.where(act, m1, m).astype(dtype),
            np.where(act, v1, v).astype(dtype))


def hyper_block(hp, t, grad_scale=1.0):
    """the device block gad_adam_step / gad_optim_jobs read (include/gaddpg.h section E), from Python doubles"""
    b1, b2 = hp["betas"]
    return np.array([hp["lr"], b1, b2, hp["eps"], hp["weight_decay"], 1.0 - b1 ** t, math.sqrt(1.0 - b2 ** t), grad_scale,
                     1.0 - b1, 1.0 - b2], dtype=np.float64).astype(np.float32)


# ----------------------------------------------------------------------------- target networks
def target_update(target, source, sel, tau, hard_enable, dtype):
    """sel 1: soft_update / half_soft_update (target * (1 - tau) + source * tau); sel 2: half_hard_update (target = source)
    when hard_enable; sel 0 (and sel 2 without hard_enable): untouched.  sel None: soft_update of everything."""
    dt = np.dtype(dtype).type
    t, s = (np.asarray(x, np.float64).astype(dtype) for x in (target, source))
    sel = np.ones(t.shape, np.uint8) if sel is None else np.asarray(sel)
    soft = t * dt(1.0 - tau) + s * dt(tau)
    return np.where(sel == 1, soft, np.where((sel == 2) & bool(hard_enable), s, t)).astype(dtype)


def sel_from_names(named_sizes):
    """the selector of a critic-like module: parameters named linear1..3* follow the soft update (1), linear4..6* the periodic
    hard update (2), anything else neither (0) -- core/utils.py half_soft_update / half_hard_update"""
    out = []
    for name, n in named_sizes:
        k = 1 if name[:7] in ("linear1", "linear2", "linear3") else 2 if name[:7] in ("linear4", "linear5", "linear6") else 0
        out.append(np.full(n, k, np.uint8))
    return np.concatenate(out)


# ----------------------------------------------------------------------------- log statistics
def absmax(x, include=None):
    """module_max_param / module_max_gradient over a flat buffer: max |x| (0 for nothing), NaN if any element is NaN
    (torch.abs(x).max() and np.amax propagate it).  include: elements that count (a parameter whose .grad is None gives 0)."""
    x = np.abs(np.asarray(x, np.float32))
    if include is not None:
        x = x[np.asarray(include).astype(bool)]
    return np.float32(np.amax(x)) if x.size else np.float32(0)


# ----------------------------------------------------------------------------- BatchNorm bookkeeping
def bn_running_update(mean, istd, count, eps, momentum, rmean, rvar, dtype):
    """torch.nn.BatchNorm1d's running statistics from SAVED batch statistics: mean and istd = 1 / sqrt(var_biased + eps)
    (float32).  var_biased is rebuilt as 1 / istd**2 - eps (clamped at 0), made unbiased with n / (n - 1) (n = 1: torch
    refuses to train; the biased variance is used), running = (1 - momentum) * running + momentum * batch."""
    dt = np.dtype(dtype).type
    mean, istd, count, rmean, rvar = (np.asarray(x, np.float64).astype(dtype) for x in (mean, istd, count, rmean, rvar))
    var = np.maximum(dt(1.0) / (istd * istd) - dt(eps), dt(0))
    unb = np.where(count > 1, var * count / np.maximum(count - dt(1), dt(1)), var)
    return ((dt(1.0 - momentum) * rmean + dt(momentum) * mean).astype(dtype),
            (dt(1.0 - momentum) * rvar + dt(momentum) * unb).astype(dtype))


def bn_eval_affine(gamma, beta, rmean, rvar, eps, dtype):
    """eval-mode BatchNorm as an affine map: scale = gamma / sqrt(running_var + eps), shift = beta - running_mean * scale"""
    dt = np.dtype(dtype).type
    gamma, beta, rmean, rvar = (np.asarray(x, np.float64).astype(dtype) for x in (gamma, beta, rmean, rvar))
    sc = gamma / np.sqrt(rvar + dt(eps))
    return sc.astype(dtype), (beta - rmean * sc).astype(dtype)


# ----------------------------------------------------------------------------- the yardstick
def rel_err(got, r64):
    """max |got - r64| / max |r64| (max-norm; 0 / 0 = 0)"""
    got, r64 = np.asarray(got, np.float64), np.asarray(r64, np.float64)
    scale = np.abs(r64).max() if r64.size else 0.0
    if scale == 0.0:
        return float(np.abs(got).max()) if got.size else 0.0
    return float(np.abs(got - r64).max() / scale)


FLOOR = 1e-6          # the head-loss gate's floor (tests/test_gpu_head_losses.py)


def within(what, got, r64, r32, floor=FLOOR):
    """the head-loss yardstick: err(got) <= max(3 x err(r32), floor), both relative to max |r64|; -> (err, err32) for logs"""
    assert np.asarray(got).shape == np.asarray(r64).shape, (what, np.asarray(got).shape, np.asarray(r64).shape)
    assert not np.isnan(np.asarray(got, np.float64)).any(), "%s: NaN left in an output" % what
    e, e32 = rel_err(got, r64), rel_err(r32, r64)
    assert e <= max(3.0 * e32, floor), "%s: max err / max|f64| = %.3e, float32 reference %.3e (ratio %.1f)" % (
        what, e, e32, e / max(e32, 1e-300))
    return e, e32


# ----------------------------------------------------------------------------- inputs
def injection(rng, n, minus_frac=0.05):
    """m2p: a random injection of n master elements into a packed buffer 1.5 x as long (so some packed slots have no master
    element), about minus_frac of the entries -1 (a master element without a packed slot).  -> (m2p int32, packed_n)"""
    packed_n = n + (n + 1) // 2 + 1
    m2p = rng.permutation(packed_n)[:n].astype(np.int32)
    if minus_frac:
        m2p[rng.random(n) < minus_frac] = -1
    return m2p, packed_n


def group_mask(rng, n, values=(0, 1)):
    """uint8 mask over n elements: aligned groups of four alternate between all-zero, mixed, and random -- what a merged
    16-byte store has to get right"""
    m = rng.choice(np.asarray(values, np.uint8), size=n)
    q = np.arange(n) // 4
    full = q < n // 4
    m[full & (q % 3 == 0)] = 0
    mixed = full & (q % 3 == 1)
    m[mixed] = np.array([values[-1], 0, values[1], 0], np.uint8)[np.arange(n)[mixed] % 4]
    return m.astype(np.uint8)

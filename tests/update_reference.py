"""What the tests of the update rules share (the sharded step's: tests/test_distributed_update_cpu.py under gloo,
tests/test_gpu_distributed_update.py under RCCL; the fused launches' and `ops.svgd_update`'s at partial-tile shapes:
tests/test_gpu_phi.py): a torch restatement of `ops.svgd_update` for CPU tensors, the fp64
reference of one update (torch.optim.Adam itself; the reference's two Adagrad lines), and the rounding bounds of the fp32
arithmetic.  Not a test module.

Why the reference is driven by the velocity the step itself reduced (`last_v_rows`), not by an independent run's: Adam and
Adagrad divide by the root of the second moment, so a last-bit difference in a velocity entry near zero comes out of an
independent run as a difference of the order of lr.  The velocity is pinned to the oracle on its
own, at the project's phi tolerance, and the update is pinned to the fp64 formulas on that velocity and on the operands the
step had (particles and state before the step), at the rounding of one update.

Rounding counts (fp32 roundings on the way from the operands to each output, every one at most 2^-24 of the magnitude
named; a scalar formed in fp64 and rounded once counts as one rounding):
  manual   X: v*mask 1, lr 1, lr*v and the difference (fused) 1                  -> 3 of |x| + lr |v|
  Adagrad  sum: v*mask 1 (twice in v^2: 2), fused multiply-add 1                 -> 3 of the new sum
           v_applied: sum 3 and + 1e-12 1 under the root (halved: 2), root 1, v*mask 1, quotient 1   -> 5 of |v_applied|
           X: v_applied 5, lr 1, fused multiply-add 1                            -> 7 of |x| + lr |v_applied|
  Adam     exp_avg: v*mask 1, v - m 1, 1-beta1 1, fused multiply-add 1           -> 4 of |m_old| + |v|
           exp_avg_sq: v*mask twice 2, v^2 1, 1-beta2 1, its product 1, beta2 1, beta2*q 1, sum 1   -> 8 of the new q
           X: m 4; denominator: q 8 and the root (halved: 4) 1, 1/sqrt(bc2) 1, fused multiply-add with eps 1 -> 7;
              quotient 1, step size 1, fused multiply-add 1                      -> 4 + 7 + 3 = 14
              of |x| + step_size |m / (sqrt(q)/sqrt(bc2) + eps)|, the magnitude this bound is set in.
              m's four roundings are of |m_old| + |v| (the exp_avg bound above), and |m| = |(1-w) m_old + w v| is smaller
              than that: by a factor of at most 1/w where m_old and v share their sign, by any factor where they cancel.
              The bound that follows from the arithmetic alone is therefore 10 of |x| + term plus 4 step_size
              (|m_old| + |v|) / denominator, which is never below the one asserted: the assertion is the stricter of
              the two, holds with a margin of 3 or more on every entry of these runs (the figures are printed), and
              would fail, not pass, on an entry where cancellation made the difference matter.
"""
import numpy as np
import torch

U = 2.0 ** -24
COUNT = {"manual_X": 3, "adagrad_sum": 3, "adagrad_v": 5, "adagrad_X": 7, "adam_m": 4, "adam_q": 8, "adam_X": 14}


def torch_update(v, X, lr, mask=None, adagrad_state=None, adam=None, inplace=False, want_v=True):
    """`ops.svgd_update` restated with torch, in fp32, for the gloo rehearsal's CPU tensors: same arguments, same in-place
    state, same return.  (Adam's scalars in fp64 and rounded once, as torch.optim.Adam and the kernel form them.)"""
    n = v.shape[0]
    g = v.detach().to(torch.float32).reshape(n, -1)
    x = X.detach().to(torch.float32).reshape(n, -1)
    if mask is not None:
        g = g * torch.broadcast_to(torch.as_tensor(mask, dtype=torch.float32), v.shape).reshape(n, -1)
    if adagrad_state is not None:
        adagrad_state.add_(g * g)
        g = g / torch.sqrt(adagrad_state + 1e-12)
    if adam is not None:
        b1, b2 = adam.betas
        t = adam.t_host + 1
        adam.exp_avg.lerp_(g, 1.0 - b1)
        adam.exp_avg_sq.mul_(b2).addcmul_(g, g, value=1.0 - b2)
        step_size = lr / (1.0 - b1 ** t)
        denom = adam.exp_avg_sq.sqrt() * float(1.0 / np.sqrt(1.0 - b2 ** t)) + adam.eps
        x_new = x - step_size * (adam.exp_avg / denom)
        adam.step += 1
        adam.t_host = t
    else:
        x_new = x - lr * g
    return (g.reshape(v.shape) if want_v else None), x_new.reshape(X.shape)


def reference_update(mode, v, x, lr, mask, state, t, betas=(0.9, 0.999), eps=1e-8):
    """One update in fp64 from fp64 copies of the step's operands: v the reduced velocity, x the particles and `state` the
    optimizer state BEFORE the step (dict of arrays: "adagrad", or "exp_avg" / "exp_avg_sq"), t the number of updates done
    before it.  Adam is torch.optim.Adam itself, its state set to the operands.  -> (x_new, v_applied, new state)"""
    x = np.asarray(x, np.float64)
    v = np.asarray(v, np.float64).reshape(x.shape)
    if mask is not None:
        v = v * np.broadcast_to(np.asarray(mask, np.float64), x.shape)
    if mode == "manual":
        return x - lr * v, v, {}
    if mode == "adagrad":  # the reference's two lines (svgd.py:110-113)
        inertia = np.asarray(state["adagrad"], np.float64).reshape(v.shape) + v ** 2
        va = v / np.sqrt(inertia + 1e-12)
        return x - lr * va, va, {"adagrad": inertia}
    p = torch.nn.Parameter(torch.tensor(x, dtype=torch.float64))
    opt = torch.optim.Adam([p], lr=lr, betas=betas, eps=eps)
    opt.state[p] = {"step": torch.tensor(float(t)),
                    "exp_avg": torch.tensor(np.asarray(state["exp_avg"], np.float64).reshape(v.shape)),
                    "exp_avg_sq": torch.tensor(np.asarray(state["exp_avg_sq"], np.float64).reshape(v.shape))}
    p.grad = torch.tensor(v)
    opt.step()
    st = opt.state[p]
    assert int(st["step"]) == t + 1
    return p.detach().numpy(), v, {"exp_avg": st["exp_avg"].numpy(), "exp_avg_sq": st["exp_avg_sq"].numpy()}


def check_update(mode, got_x, got_state, v, x, lr, mask, state, t, betas=(0.9, 0.999), eps=1e-8, where="", got_v=None):
    """Asserts one step's new particles and state against `reference_update` within the rounding bounds of the module
    docstring; prints each figure (largest error over its bound) before it asserts.  `got_v`: the velocity the launch
    stored (after mask and Adagrad), asserted too where given: COUNT["adagrad_v"] roundings of |v_applied| under Adagrad,
    the one rounding of v * mask otherwise."""
    x_ref, va, st_ref = reference_update(mode, v, x, lr, mask, state, t, betas, eps)
    f = lambda a, like: np.asarray(a, np.float64).reshape(np.shape(like))
    checks = []
    if mode == "manual":
        checks.append(("X", f(got_x, x_ref), x_ref, COUNT["manual_X"] * U * (np.abs(x) + lr * np.abs(va))))
    elif mode == "adagrad":
        s = st_ref["adagrad"]
        checks.append(("adagrad", f(got_state["adagrad"], s), s, COUNT["adagrad_sum"] * U * s))
        checks.append(("X", f(got_x, x_ref), x_ref, COUNT["adagrad_X"] * U * (np.abs(x) + lr * np.abs(va))))
    else:
        m, q = st_ref["exp_avg"], st_ref["exp_avg_sq"]
        m_old = np.asarray(state["exp_avg"], np.float64).reshape(m.shape)
        t1 = t + 1
        step_size = lr / (1.0 - betas[0] ** t1)
        term = step_size * np.abs(m / (np.sqrt(q) / np.sqrt(1.0 - betas[1] ** t1) + eps))
        checks.append(("exp_avg", f(got_state["exp_avg"], m), m, COUNT["adam_m"] * U * (np.abs(m_old) + np.abs(va))))
        checks.append(("exp_avg_sq", f(got_state["exp_avg_sq"], q), q, COUNT["adam_q"] * U * q))
        checks.append(("X", f(got_x, x_ref), x_ref, COUNT["adam_X"] * U * (np.abs(np.asarray(x, np.float64)) + term)))
    if got_v is not None:
        checks.append(("v_applied", f(got_v, va), va, (COUNT["adagrad_v"] if mode == "adagrad" else 1) * U * np.abs(va)))
    for name, got, ref, bound in checks:
        err = np.abs(got - ref)
        worst = float((err / np.maximum(bound, 1e-300)).max()) if err.max() > 0 else 0.0
        print(f"{where} {mode} {name}: largest error / bound = {worst:.3f} (max |error| {err.max():.3e})")
        assert (err <= bound).all(), (where, mode, name, worst)

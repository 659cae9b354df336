"""How large the tensors are that the GPU tests compare (not collected: no test_ prefix).  `python tests/tensor_magnitudes.py`
prints the tables of tests/README.md: max|.| / rms of every backward tensor from the float64 oracles, at the weights and
batches the GPU tests use.  A bound of the form tol x max(1, max|want|) is absolute for every tensor below 1."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.join(os.path.dirname(HERE), "oracle"), os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import ga3c_oracle as o  # noqa: E402


def _cell(t):
    t = np.asarray(t, np.float64)
    return "%.1e / %.1e" % (np.max(np.abs(t)), np.sqrt(np.mean(t * t)))


def _table(title, columns, rows):
    print("\n%s\n" % title)
    print("| tensor | " + " | ".join(columns) + " |")
    print("|---|" + "---|" * len(columns))
    for name, cells in rows:
        print("| `%s` | " % name + " | ".join(cells) + " |")


def image_net():
    import test_gpu_parity as tp
    for num_actions in (6, 18):
        sizes, cols = (1, 5, 37, 128), {}
        for bsz in sizes:
            _, x, a, y = tp._batch(bsz, num_actions, 300 + bsz)
            _, cols[bsz] = o.loss_and_grads(o.init_params(num_actions), x.astype(np.float64), y, a.astype(np.float64), 0.01)
        names = ("dz", "dv", "dd1", "dn2", "dn1") + o.PARAM_ORDER
        _table("image net, A = %d, init_params, rows of test_gpu_parity._batch(B, A, 300 + B), beta = 0.01 (max / rms)" % num_actions,
               ["B = %d" % b for b in sizes], [(n, [_cell(cols[b][n]) for b in sizes]) for n in names])


def vector_net():
    import mlp_oracle as m
    import test_gpu_vector_net as tv
    for state_dim, num_actions in ((3, 1), (7, 3)):
        params = tv._params(state_dim, num_actions)
        sizes, cols = (1, 16, 128, 1024), {}
        for bsz in sizes:
            x, y, a = tv._batch(params, bsz, state_dim, num_actions, 100 + bsz)
            _, cols[bsz] = m.loss_and_grads(params, x.astype(np.float64), y.astype(np.float64), a.astype(np.float64), 0.01)
        names = ("dv", "dz", "dd1", "dpd4", "dpd3", "dpd2", "dpd1") + m.PARAM_ORDER
        _table("vector net, state_dim = %d, A = %d, the weights and rows of test_gpu_vector_net (max / rms)" % (state_dim, num_actions),
               ["B = %d" % b for b in sizes], [(n, [_cell(cols[b][n]) for b in sizes]) for n in names])


def vector_saturated():
    import mlp_oracle as m
    import vector_limit_cases as vc
    cols = {}
    for S, A in vc.SATURATED:
        x, y, a = vc.saturated_batch(S, A)
        _, cols[S, A] = m.loss_and_grads(vc.saturated_params(S, A), *vc.f64(x, y, a), vc.BETA)
    names = ("dv", "dz", "dd1", "dpd4", "dpd3", "dpd2", "dpd1") + m.PARAM_ORDER
    _table("vector net with a saturated head (logits_p/out_x/w, out_y/w x %g), B = %d, the weights and rows of "
           "test_gpu_vector_limits (max / rms)" % (vc.SAT_SCALE, vc.SAT_B), ["S = %d, A = %d" % sa for sa in vc.SATURATED],
           [(n, [_cell(cols[sa][n]) for sa in vc.SATURATED]) for n in names])


def ddpg():
    import ddpg_oracle as d
    import test_gpu_ddpg as td
    for S, A in td.SHAPES:
        sizes, cols = (1, 17, 128, 300), {}
        for B in sizes:
            noise = np.linspace(-0.2, 0.3, A).astype(np.float32)
            online, target, batch = td._case(S, A, B, 100 + B + S, stats=True, noise=noise)
            st = d.new_state(online, target)
            out = d.train_step(st, *td._f64(batch), td.LR, noise.astype(np.float64), stop_after=4)
            fc, fa = out["critic_fwd"], out["actor_fwd"]
            t = {"dq": out["dq"], "c_dt": fc["dt"], "c_dn1": fc["dn1"], "g": out["g"], "do": fa["do"], "a_dn2": fa["dn2"],
                 "a_dn1": fa["dn1"]}
            t.update({"grad " + k: out["critic_grads"][k] for k in d.CRITIC_TRAINABLE if k != d.DEAD})
            t.update({"grad " + k: out["actor_grads"][k] for k in d.ACTOR_TRAINABLE})
            cols[B] = t
        _table("DDPG, S = %d, A = %d, the weights and rows of test_gpu_ddpg.test_every_intermediate_and_gradient (max / rms)" % (S, A),
               ["B = %d" % b for b in sizes], [(n, [_cell(cols[b][n]) for b in sizes]) for n in cols[sizes[0]]])


if __name__ == "__main__":
    image_net()
    vector_net()
    vector_saturated()
    ddpg()

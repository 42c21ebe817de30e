"""Cases shared by tests/test_ars_cpu.py and tests/test_ars_gpu.py: update cases with distinct scores, sb3_contrib's update lines restated in
torch float64, the crafted return vectors, and random policies of every network the tests run."""
import numpy as np

# (n_delta, n_top) of the update cases: n_top = n_delta, n_top < n_delta, n_top = 1, n_delta = 1
UPDATE_CASES = [(8, 8), (8, 3), (8, 1), (1, 1)]
# network tag -> (kind, D, h1, h2, P)
NETS = {
    "pst-64-64": ("MlpPolicy", 63, 64, 64, 20), "ppl-64-64": ("MlpPolicy", 162, 64, 64, 50), "pst-33-17": ("MlpPolicy", 63, 33, 17, 20),
    "ppl-33-17": ("MlpPolicy", 162, 33, 17, 50), "pst-256-256": ("MlpPolicy", 63, 256, 256, 20), "ppl-256-256": ("MlpPolicy", 162, 256, 256, 50),
    "pst-linear": ("LinearPolicy", 63, 0, 0, 20), "ppl-linear": ("LinearPolicy", 162, 0, 0, 50),
}


def update_case(n_delta, n_top, n_params=57, seed=0):
    """theta, delta, returns [2 n_delta] with pairwise distinct scores max(r+, r-)"""
    rng = np.random.default_rng(1000 * n_delta + 10 * n_top + seed)
    theta = rng.normal(0.0, 0.3, n_params).astype(np.float32)
    delta = rng.normal(size=(n_delta, n_params)).astype(np.float32)
    returns = rng.normal(-50.0, 20.0, 2 * n_delta)
    return dict(theta=theta, delta=delta, returns=returns, n_delta=n_delta, n_top=n_top, lr=0.02)


def scores(returns):
    n = len(returns) // 2
    return np.maximum(returns[:n], returns[n:])


def torch_update(case):
    """sb3_contrib's ARS._do_one_update lines, float64: (new theta, sigma_R, step, top_idx)"""
    import torch as th
    theta, delta = th.from_numpy(case["theta"].astype(np.float64)), th.from_numpy(case["delta"].astype(np.float64))
    r = th.from_numpy(np.asarray(case["returns"], np.float64))
    n_delta, n_top = case["n_delta"], case["n_top"]
    plus_returns, minus_returns = r[:n_delta], r[n_delta:]
    top_returns, _ = th.max(th.vstack((plus_returns, minus_returns)), dim=0)
    top_idx = th.argsort(top_returns, descending=True)[:n_top]
    plus_returns, minus_returns, deltas = plus_returns[top_idx], minus_returns[top_idx], delta[top_idx]
    return_std = th.cat([plus_returns, minus_returns]).std()
    step_size = case["lr"] / (n_top * return_std + 1e-6)
    new = theta + step_size * ((plus_returns - minus_returns) @ deltas)
    return new.numpy(), float(return_std), float(step_size), top_idx.numpy()


def crafted_returns(n_delta=4):
    """name -> returns [2 n_delta]: ties (equal scores), all equal, a NaN, an infinity"""
    base = np.array([3.0, -1.0, 7.5, 2.0, 0.5, 4.0, 4.0, 2.5][:2 * n_delta], np.float64)
    ties = np.array([5.0, 1.0, 5.0, 0.0, 2.0, 5.0, 3.0, 5.0][:2 * n_delta], np.float64)   # every score is 5
    nan, inf = base.copy(), base.copy()
    nan[5], inf[2] = np.nan, -np.inf
    return {"plain": base, "ties": ties, "equal": np.full(2 * n_delta, -12.5), "nan": nan, "inf": inf}


def random_theta(tag, seed=0, scale=1.0):
    """A policy's parameter vector with torch.nn.Linear-style uniform(-1/sqrt(in), 1/sqrt(in)) arrays (times `scale`), float32"""
    from ev2gym_amd import _abi
    kind, D, h1, h2, P = NETS[tag]
    rng = np.random.default_rng(seed + 17 * D + P)
    parts = []
    fan = 1
    for s in _abi.ars_param_shapes(kind, D, h1, h2, P):
        if len(s) == 2:
            fan = s[1]
        k = scale / np.sqrt(fan)
        parts.append(rng.uniform(-k, k, s).astype(np.float32).ravel())
    return np.concatenate(parts)

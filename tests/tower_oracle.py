"""Float64 forward oracle of the default (64-wide) towers - TEST INFRASTRUCTURE.

``oracle/ppo_oracle.py``'s ``tower_forward`` is plain torch, so the same function run on float64 copies of the parameters
and inputs gives a reference ``ref64`` whose own rounding is negligible next to fp32; the float32 run of the same function
is ``ref32``, the reference implementation's own distance from it.  A kernel output ``got`` passes when

    |got - ref64| <= atol + rtol |ref64| + k max|ref32 - ref64|

(the form of ``tests/test_layernorm_adversarial_gpu.py``).  ``head_fields`` derives what the kernels return from a tower
output - values, log-probs, entropies, sampled actions - in either precision, so the bar applies to every field.

``draw_tower`` draws parameters whose W1 columns are all O(1 / sqrt(D)) (the last ones scaled up), so that on N(0, 1)
observations the last columns of a row move every output; ``tail_sensitivity`` measures how far the float64 outputs move
when those columns are zeroed - a test asserts that a kernel dropping them could not pass its bar.
Nothing under ``oracle/`` is changed (the goldens keep reproducing)."""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch

from oracle import philox as px
from oracle import ppo_oracle as po

LOG_SQRT_2PI = 0.91893853320467274178


def spec(obs_dim: int, head: str, n: int) -> po.TowerSpec:
    """head "disc" (Categorical over n) or "box" (DiagGaussian of n dimensions)."""
    return po.TowerSpec(obs_dim, n, po.HEAD_CATEGORICAL if head == "disc" else po.HEAD_GAUSSIAN)


def critic_spec(obs_dim: int) -> po.TowerSpec:
    return po.TowerSpec(obs_dim, 1, po.HEAD_VALUE)


def draw_tower(sp: po.TowerSpec, rs: np.random.RandomState) -> torch.Tensor:
    """Flat float32 parameters in the engine's layout (``TowerSpec.sizes``).  Pre-activations of fc1 are O(1) on N(0, 1)
    inputs; W1's last 4 columns carry twice the scale of the others (a dropped tail moves every output); LayerNorm gains
    around 1, biases, betas and log-stds spread so that no term is degenerate."""
    D, H, K = sp.obs_dim, sp.hidden, sp.n_out
    parts = {
        "W1": rs.randn(H, D) / np.sqrt(D),
        "b1": 0.3 * rs.randn(H), "g1": 1.0 + 0.2 * rs.randn(H), "be1": 0.1 * rs.randn(H),
        "W2": rs.randn(H, H) / np.sqrt(H),
        "b2": 0.1 * rs.randn(H), "g2": 1.0 + 0.2 * rs.randn(H), "be2": 0.1 * rs.randn(H),
        "W3": 0.6 * rs.randn(K, H) / np.sqrt(H), "b3": 0.2 * rs.randn(K),
        "logstd": rs.uniform(-1.0, 0.5, K),
    }
    parts["W1"][:, max(0, D - 4):] *= 2.0
    flat = [parts[name].reshape(-1) for name, _ in sp.sizes()]
    return torch.as_tensor(np.concatenate(flat), dtype=torch.float32)


def forward(sp: po.TowerSpec, theta: torch.Tensor, x, dtype) -> torch.Tensor:
    """``po.tower_forward`` with parameters and inputs cast to ``dtype``."""
    with torch.no_grad():
        return po.tower_forward(sp, theta.to(dtype), torch.as_tensor(np.asarray(x)).to(dtype))


def logstd(sp: po.TowerSpec, theta: torch.Tensor, dtype) -> torch.Tensor:
    return sp.split(theta.to(dtype))["logstd"]


def categorical_cdf(logits: np.ndarray):
    """(masked) logits [B, n] float64 -> (p, cumsum p) in float64."""
    lg = np.asarray(logits, dtype=np.float64)
    p = np.exp(lg - lg.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    return p, np.cumsum(p, axis=-1)


def head_fields(sp: po.TowerSpec, theta: torch.Tensor, x, dtype, masks=None, actions=None, eps=None) -> Dict:
    """What the kernels return for inputs x, in ``dtype``:

    * "out": the head (logits, masked with -6e4 like ``distributions.py:70-71``, or the Gaussian mean);
    * categorical: "logp_all" [B, n] (log-softmax), "ent" [B];
    * Gaussian: "ent" [B] (sum over dimensions), and with ``eps`` ([B, n] normals) "act" = mean + std eps and its "logp";
    * with ``actions`` (the kernel's or the stored ones): "logp" of those actions."""
    out = forward(sp, theta, x, dtype)
    r = {}
    if sp.head == po.HEAD_CATEGORICAL:
        if masks is not None:
            out = torch.where(torch.as_tensor(np.asarray(masks)) == 0, torch.full_like(out, -6e4), out)
        lsm = torch.log_softmax(out, dim=-1)
        r["logp_all"] = lsm.numpy()
        r["ent"] = (-(lsm.exp() * lsm).sum(-1)).numpy()
        if actions is not None:
            a = torch.as_tensor(np.asarray(actions).reshape(-1).astype(np.int64))
            r["logp"] = lsm.gather(1, a[:, None]).numpy()
    elif sp.head == po.HEAD_GAUSSIAN:
        ls = logstd(sp, theta, dtype)
        std = ls.exp()
        r["ent"] = (0.5 + LOG_SQRT_2PI + ls).sum().expand(out.shape[0]).clone().numpy()
        if eps is not None:
            e = torch.as_tensor(np.asarray(eps)).to(dtype)
            act = out + std * e
            r["act"] = act.numpy()
            r["logp"] = (-(e * e) / 2 - ls - LOG_SQRT_2PI).numpy()  # = Normal(mean, std).log_prob(act) in real arithmetic
        if actions is not None:
            a = torch.as_tensor(np.asarray(actions)).to(dtype)
            r["logp"] = (-((a - out) ** 2) / (2 * std * std) - ls - LOG_SQRT_2PI).numpy()
    r["out"] = out.numpy()
    return r


def bar(ref64, ref32, atol: float, rtol: float, k: float) -> np.ndarray:
    ref64, ref32 = np.asarray(ref64, np.float64), np.asarray(ref32, np.float64)
    return atol + rtol * np.abs(ref64) + k * np.max(np.abs(ref32 - ref64), initial=0.0)


class Ledger:
    """Collects every comparison of a sweep: the worst |got - ref64|, |ref32 - ref64| and (got error) / bar per field, and
    the cases that failed - one assertion at the end names all of them."""

    def __init__(self, atol: float, rtol: float, k: float):
        self.atol, self.rtol, self.k = atol, rtol, k
        self.worst: Dict[str, list] = {}
        self.failures = []

    def check(self, case: str, field: str, got, ref64, ref32) -> np.ndarray:
        """Returns the bar (elementwise); records a failure when any element is outside it."""
        got, ref64, ref32 = (np.asarray(a, np.float64) for a in (got, ref64, ref32))
        b = bar(ref64, ref32, self.atol, self.rtol, self.k)
        err = np.abs(got - ref64)
        err = np.where(np.isnan(got), np.inf, err)
        ratio = float(np.max(err / b, initial=0.0))
        w = self.worst.setdefault(field, [0.0, 0.0, 0.0, ""])
        w[0] = max(w[0], float(np.max(err, initial=0.0)))
        w[1] = max(w[1], float(np.max(np.abs(ref32 - ref64), initial=0.0)))
        if ratio > w[2]:
            w[2], w[3] = ratio, case
        if ratio > 1.0:
            i = int(np.argmax(err / b))
            self.failures.append("%s %s: |got - ref64| = %.3g at flat index %d (bar %.3g; got %.7g, ref64 %.7g), %d of %d "
                                 "outside" % (case, field, err.reshape(-1)[i], i, b.reshape(-1)[i], got.reshape(-1)[i],
                                              ref64.reshape(-1)[i], int((err > b).sum()), err.size))
        return b

    def fail(self, msg: str) -> None:
        self.failures.append(msg)

    def report(self) -> str:
        return "\n".join("  %-10s max|got-ref64| %.3g  max|ref32-ref64| %.3g  worst err/bar %.3f (%s)" % (f, *w)
                         for f, w in sorted(self.worst.items()))

    def assert_ok(self) -> None:
        print("\n" + self.report())
        assert not self.failures, "%d failed comparisons:\n%s\nworst per field:\n%s" % (
            len(self.failures), "\n".join(self.failures[:40]), self.report())


def tail_columns(D: int) -> slice:
    """The columns a dropped tail would lose: those past 64, or the last 4 of a narrower observation."""
    return slice(64, None) if D > 64 else slice(max(0, D - 4), None)


def tail_sensitivity(sp: po.TowerSpec, theta: torch.Tensor, x, masks=None) -> np.ndarray:
    """float64 head output with the tail columns of x zeroed minus the true one."""
    x = np.array(x, dtype=np.float64, copy=True)
    ref = head_fields(sp, theta, x, torch.float64, masks)["out"]
    x[:, tail_columns(sp.obs_dim)] = 0.0
    return head_fields(sp, theta, x, torch.float64, masks)["out"] - ref


def check_sensitivity(led: Ledger, case: str, field: str, moved: np.ndarray, b: np.ndarray, factor: float = 20.0):
    """A kernel that dropped the tail columns would have been off by ``moved``: require max |moved| / bar >= factor."""
    r = float(np.max(np.abs(moved) / b, initial=0.0))
    if not r >= factor:
        led.fail("%s %s: zeroing the tail columns moves the float64 output by only %.3g bars (< %g) - the case cannot see "
                 "a dropped tail" % (case, field, r, factor))


def sample_edge_ok(got_a: np.ndarray, u: np.ndarray, logits64: np.ndarray, masks, tol: float) -> np.ndarray:
    """Per row: is the kernel's sampled action ``got_a`` the float64 inverse-CDF sample of uniform ``u`` - or, where u sits
    within ``tol`` of a CDF edge, an allowed action whose CDF interval reaches u within tol?"""
    p, cdf = categorical_cdf(logits64)
    ut = np.asarray(u, np.float64).reshape(-1)  # sum(p) = 1 in float64
    a = np.asarray(got_a).reshape(-1).astype(np.int64)
    B, n = p.shape
    inside = (a >= 0) & (a < n)
    ai = np.clip(a, 0, n - 1)
    hi = cdf[np.arange(B), ai]
    lo = np.where(ai > 0, cdf[np.arange(B), np.maximum(ai - 1, 0)], 0.0)
    allowed = np.ones(B, dtype=bool) if masks is None else np.asarray(masks)[np.arange(B), ai] != 0
    # exact: lo <= u < hi; near an edge: within tol of the interval
    return inside & allowed & (ut >= lo - tol) & (ut < hi + tol)


def philox_uniforms(seed: int, rows: np.ndarray, step: int) -> np.ndarray:
    """The categorical sampler's uniforms (``orl_heads.h`` sample_head): u01 of philox(seed, row, 0, step, hi(step) << 8).x"""
    x, _, _, _ = px.philox4x32_10(seed, rows.astype(np.uint32), 0, step & 0xFFFFFFFF, (step >> 32) << 8)
    return px.u01(x)


def philox_normals(seed: int, rows: np.ndarray, step: int, n: int) -> np.ndarray:
    """The Gaussian sampler's normals (``orl_heads.h`` sample_head): block b of 4 from philox(seed, row, 0, step,
    (hi(step) << 8) | b), Box-Muller of (x, y) and (z, w) - here in float64 from the same 32-bit words."""
    cols = []
    for b in range((n + 3) // 4):
        x, y, z, w = px.philox4x32_10(seed, rows.astype(np.uint32), 0, step & 0xFFFFFFFF, ((step >> 32) << 8) | b)
        for s, c in ((x, y), (z, w)):
            u1 = ((s >> np.uint32(8)).astype(np.float64) + 1.0) / 16777216.0
            u2 = (c >> np.uint32(8)).astype(np.float64) / 16777216.0
            rad = np.sqrt(-2.0 * np.log(u1))
            cols += [rad * np.cos(2 * np.pi * u2), rad * np.sin(2 * np.pi * u2)]
    return np.stack(cols[:n], axis=-1)

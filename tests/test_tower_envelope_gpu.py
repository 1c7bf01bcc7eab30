"""The default towers' forward kernels against a float64 oracle across every observation width and head they accept.

``check_net`` (``csrc/orl_act.hip``) admits obs_dim 1..256 and policy heads of 1..16 outputs; which kernel instance runs
depends on the width (fc1's k-steps, the register / LDS operand splits at 8 and 16 k-steps) and on LDS fit.  The golden
cases only cover obs 4 - 6 with 1 - 3 outputs, so every call here is swept over

* widths 1 .. 256: the COOP_SMALL_DP = 8 path, single-k-step instances, the policy waves' register / LDS split at 32
  columns, the 16-k-step (64-column) register prefetch of the critic paths, and the kernel / refusal boundaries of the
  fused rollout (chain kernel obs <= 64; lock-step kernel up to 156 with <= 2 outputs, 152 with more);
* Discrete 2 .. 16 with and without action masks (the NO = 2 / 8 / 16 instances, MFMA wide heads above 4 outputs) and
  Box 1 .. 16;

and compared with ``tests/tower_oracle.py``: float64 runs of ``oracle/ppo_oracle.py``'s tower with the bar
|got - ref64| <= atol + rtol |ref64| + K max|ref32 - ref64|.  Every case also asserts that zeroing the observation's tail
columns (those past 64, or the last 4 of a narrower row) would move the float64 outputs by at least 20 bars, so a kernel
that drops or misreads them cannot pass.

Measured on one MI355X over the whole sweep, max |got - ref64| (in brackets max |ref32 - ref64|, torch's float32 forward):

* ``orl_act_step``: values 1.1e-6 (8.8e-7), log-probs 1.2e-6 (8.8e-7), continuous actions 1.0e-6 (8.5e-7);
* ``orl_evaluate_actions``: log-probs 5.3e-6 (3.8e-6), per-row entropies 3.3e-6 (2.5e-6), values 9.6e-7 (8.2e-7);
* ``orl_critic_values``: 9.3e-7 (8.7e-7);
* the fused rollout, both kernels: log-probs 3.9e-6 (1.4e-6), continuous actions 2.1e-6 (9.7e-7), next_value 6.9e-7
  (8.0e-7), value_preds 8.9e-7 (9.9e-7).

The bar is ATOL 1e-5, RTOL 1e-5, K 2: the largest error measured (5.3e-6) is about half of ATOL alone, and the worst
comparison of the sweep used 0.15 of its bar (a rollout's continuous action at obs 69, Box(6)).

On the parent commit's library the sweep failed at exactly these places:

* the chain kernel at obs 65 - 68 with <= 2 outputs: its critic waves read 16 k-steps (64 columns) of the observation
  into registers and dropped the rest: value_preds and next_value off by up to 1.19 (obs 68, Discrete(2)) - about 4e4
  bars.  It now hands observations wider than 64 columns to the lock-step kernel;
* ``orl_critic_values`` at every width > 64: its operand select returned the first k-step's column for every k-step
  past 16 - values off by up to 2.98 (obs 152).  k-steps past the 16 prefetched ones now read global memory like
  ``orl_act_step``'s critic.  (test_kernels_gpu.py::test_batched_critic_values_equal_the_act_step_critic failed too,
  at obs 65, 100 and 256.)
Needs a MI355X."""
import numpy as np
import pytest
import torch

from oracle import ppo_oracle as po
from tests import tower_oracle as TO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ATOL, RTOL, K = 1e-5, 1e-5, 2.0
CDF_TOL = 1e-5   # a uniform this close (float64) to a CDF edge may land on either side in fp32
ENT_TOL = 1e-5   # dist_entropy (a mean over rows)

WIDTHS = [1, 2, 3, 4, 5, 7, 8, 9, 12, 16, 17, 31, 32, 33, 60, 63, 64, 65, 66, 68, 69, 100, 128, 152, 153, 156, 157, 256]
NARROW = [("disc", 2, False), ("box", 1, False), ("disc", 2, True), ("box", 2, False)]
WIDE = [("disc", 9, True), ("disc", 16, False), ("box", 16, False), ("disc", 9, False), ("disc", 16, True)]
MIDDLE = [("disc", 3, True), ("disc", 4, False), ("disc", 5, True), ("disc", 8, False), ("box", 3, False),
          ("box", 6, False), ("disc", 3, False), ("disc", 5, False), ("disc", 8, True), ("disc", 4, True)]
BATCHES = [37, 1000, 1, 37, 1000]

# every width with a narrow head and a wide one; every other head at a width <= 8, one in 17..64 and one above 64
CASES = [(D, NARROW[i % len(NARROW)]) for i, D in enumerate(WIDTHS)] + \
        [(D, WIDE[i % len(WIDE)]) for i, D in enumerate(WIDTHS)] + \
        [(D, h) for i, h in enumerate(MIDDLE) for D in (WIDTHS[i % 7], WIDTHS[10 + i % 7], WIDTHS[17 + i % 11])]


def _coverage():
    for D in WIDTHS:
        assert any(c[0] == D and c[1][1] <= 2 for c in CASES) and any(c[0] == D and c[1][1] >= 9 for c in CASES), D
    heads = {(h, n, m) for _, (h, n, m) in CASES}
    for h in heads:
        ds = [D for D, hh in CASES if hh == h]
        assert min(ds) <= 8 and any(17 <= D <= 64 for D in ds) and max(ds) > 64, (h, ds)
    for n in (2, 3, 4, 5, 8, 9, 16):
        assert {m for h, nn, m in heads if h == "disc" and nn == n} == {False, True}, n
    assert {n for h, n, _ in heads if h == "box"} == {1, 2, 3, 6, 16}


_coverage()


def dev(x, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).to(DEV).contiguous()


@pytest.fixture(scope="module")
def ops():
    from openrl_amd import ops as _ops

    return _ops


def _name(D, head, B=None):
    h, n, m = head
    return "obs %d %s(%d)%s%s" % (D, "Discrete" if h == "disc" else "Box", n, "+masks" if m else "",
                                   "" if B is None else " B=%d" % B)


def _both_towers_fit(D, n):
    """orl_act_step / orl_evaluate_actions stage both towers in one workgroup's LDS: at obs 256 they do not fit."""
    return D <= 232


def _case_inputs(D, head, B, seed):
    h, n, m = head
    rs = np.random.RandomState(seed)
    ps, cs = TO.spec(D, h, n), TO.critic_spec(D)
    tp, tc = TO.draw_tower(ps, rs), TO.draw_tower(cs, rs)
    obs = rs.randn(B, D).astype(np.float32)
    masks = None
    if m:
        masks = (rs.rand(B, n) > 0.35).astype(np.float32)
        masks[np.arange(B), rs.randint(0, n, B)] = 1.0
    return rs, ps, cs, tp, tc, obs, masks


def _check_values(led, case, got, cs, tc, obs):
    r64 = TO.head_fields(cs, tc, obs, torch.float64)["out"]
    r32 = TO.head_fields(cs, tc, obs, torch.float32)["out"]
    b = led.check(case, "value", np.asarray(got).reshape(r64.shape), r64, r32)
    TO.check_sensitivity(led, case, "value", TO.tail_sensitivity(cs, tc, obs), b)


def test_act_step_across_the_envelope(ops):
    """orl_act_step with both towers: deterministic (argmax / mean) and teacher-forced (uniforms / normals) - values,
    actions, log-probs against float64."""
    led = TO.Ledger(ATOL, RTOL, K)
    for ci, (D, head) in enumerate(CASES):
        B = BATCHES[ci % len(BATCHES)]
        case = _name(D, head, B)
        h, n, m = head
        rs, ps, cs, tp, tc, obs, masks = _case_inputs(D, head, B, 1000 + ci)
        pnet, cnet = ops.net_desc(D, n, ps.head), ops.net_desc(D, 1, ops.HEAD_VALUE)
        a_w = 1 if h == "disc" else n
        d_obs, d_masks = dev(obs), (None if masks is None else dev(masks))
        r64 = TO.head_fields(ps, tp, obs, torch.float64, masks)
        r32 = TO.head_fields(ps, tp, obs, torch.float32, masks)
        b_out = TO.bar(r64["out"], r32["out"], ATOL, RTOL, K)
        TO.check_sensitivity(led, case, "head", TO.tail_sensitivity(ps, tp, obs, masks), b_out)
        for det in (True, False):
            forced = rs.rand(B, 1).astype(np.float32) if h == "disc" else rs.randn(B, n).astype(np.float32)
            values, actions, logp = (torch.full((B, w), np.nan, device=DEV) for w in (1, a_w, a_w))
            if _both_towers_fit(D, n):
                ops.act_step(pnet, dev(tp), cnet, dev(tc), d_obs, d_obs, d_masks, B, det, 0, 0, 0,
                             None if det else dev(forced), values, actions, logp)
            else:  # refused with a message, and the next (one-tower) calls still work
                with pytest.raises(ops.nat.NativeError, match="LDS"):
                    ops.act_step(pnet, dev(tp), cnet, dev(tc), d_obs, d_obs, d_masks, B, det, 0, 0, 0,
                                 None if det else dev(forced), values, actions, logp)
                ops.act_step(pnet, dev(tp), None, None, d_obs, None, d_masks, B, det, 0, 0, 0,
                             None if det else dev(forced), None, actions, logp)
                ops.critic_values(cnet, dev(tc), d_obs, values)
            torch.cuda.synchronize()
            c = case + (" deterministic" if det else " forced")
            _check_values(led, c, values.cpu().numpy(), cs, tc, obs)
            got_a, got_lp = actions.cpu().numpy(), logp.cpu().numpy()
            if h == "disc":
                if det:  # argmax; a near-tie (float64 gap within the bar) may go either way
                    lg = r64["out"]
                    a = got_a[:, 0].astype(np.int64)
                    ok = (a >= 0) & (a < n)
                    gap = lg.max(-1) - lg[np.arange(B), np.clip(a, 0, n - 1)]
                    ok &= gap <= 2 * b_out.max(-1)
                else:
                    ok = TO.sample_edge_ok(got_a, forced, r64["out"], masks, CDF_TOL)
                if not ok.all():
                    led.fail("%s: %d of %d sampled actions are not the float64 sample (first row %d: got %s)" % (
                        c, int((~ok).sum()), B, int(np.argmin(ok)), got_a[np.argmin(ok), 0]))
                    continue
                if masks is not None and not np.all(masks[np.arange(B), got_a[:, 0].astype(int)] == 1):
                    led.fail("%s: sampled a masked action" % c)
                a = got_a[:, 0].astype(np.int64)
                led.check(c, "logp", got_lp[:, 0], r64["logp_all"][np.arange(B), a], r32["logp_all"][np.arange(B), a])
            else:
                eps = np.zeros((B, n)) if det else forced
                f64 = TO.head_fields(ps, tp, obs, torch.float64, eps=eps)
                f32 = TO.head_fields(ps, tp, obs, torch.float32, eps=eps)
                led.check(c, "action", got_a, f64["act"], f32["act"])
                led.check(c, "logp", got_lp, f64["logp"], f32["logp"])
    led.assert_ok()


def test_evaluate_actions_across_the_envelope(ops):
    """orl_evaluate_actions with both towers: log-probs of stored actions, per-row entropies (x active mask), the
    masked-mean dist_entropy and values against float64."""
    led = TO.Ledger(ATOL, RTOL, K)
    for ci, (D, head) in enumerate(CASES):
        B = BATCHES[(ci + 1) % len(BATCHES)]
        case = _name(D, head, B)
        h, n, m = head
        rs, ps, cs, tp, tc, obs, masks = _case_inputs(D, head, B, 2000 + ci)
        pnet, cnet = ops.net_desc(D, n, ps.head), ops.net_desc(D, 1, ops.HEAD_VALUE)
        a_w = 1 if h == "disc" else n
        r64m = TO.head_fields(ps, tp, obs, torch.float64, masks)
        if h == "disc":  # stored actions: allowed ones
            p, _ = TO.categorical_cdf(r64m["out"])
            act = np.array([rs.choice(n, p=pr / pr.sum()) for pr in p + 1e-3 * (p > 0)], dtype=np.float32)[:, None]
        else:
            act = (r64m["out"] + rs.randn(B, n) * np.exp(TO.logstd(ps, tp, torch.float64).numpy())).astype(np.float32)
        active = (rs.rand(B) > 0.25).astype(np.float32)
        active[0] = 1.0
        use_active = ci % 2 == 0
        values, logp = torch.full((B, 1), np.nan, device=DEV), torch.full((B, a_w), np.nan, device=DEV)
        ent_rows, ent = torch.full((B,), np.nan, device=DEV), torch.full((1,), np.nan, device=DEV)
        args = (dev(obs), dev(obs), dev(act), None if masks is None else dev(masks), dev(active) if use_active else None, B)
        if _both_towers_fit(D, n):
            ops.evaluate_actions(pnet, dev(tp), cnet, dev(tc), *args, values, logp, ent_rows, ent)
        else:
            with pytest.raises(ops.nat.NativeError, match="LDS"):
                ops.evaluate_actions(pnet, dev(tp), cnet, dev(tc), *args, values, logp, ent_rows, ent)
            ops.evaluate_actions(pnet, dev(tp), None, None, *args, None, logp, ent_rows, ent)
            ops.critic_values(cnet, dev(tc), dev(obs), values)
        torch.cuda.synchronize()
        _check_values(led, case, values.cpu().numpy(), cs, tc, obs)
        f64 = TO.head_fields(ps, tp, obs, torch.float64, masks, actions=act)
        f32 = TO.head_fields(ps, tp, obs, torch.float32, masks, actions=act)
        b = led.check(case, "logp", logp.cpu().numpy().reshape(f64["logp"].shape), f64["logp"], f32["logp"])
        TO.check_sensitivity(led, case, "head", TO.tail_sensitivity(ps, tp, obs, masks),
                             TO.bar(f64["out"], f32["out"], ATOL, RTOL, K))
        w = active.astype(np.float64) if use_active else np.ones(B)
        led.check(case, "ent_rows", ent_rows.cpu().numpy(), f64["ent"] * w, f32["ent"] * w)
        den = w.sum() if use_active else B * (n if h == "box" else 1)
        want = float((f64["ent"] * w).sum() / den)
        if not abs(ent.item() - want) <= ENT_TOL * max(1.0, abs(want)):
            led.fail("%s: dist_entropy %.8g, float64 %.8g" % (case, ent.item(), want))
    led.assert_ok()


def test_critic_values_across_the_envelope(ops):
    """orl_critic_values (the batched value sweep) against float64 directly, at every width up to 256 and ragged row
    counts - and the width past the envelope refused, the next call unaffected."""
    led = TO.Ledger(ATOL, RTOL, K)
    for ci, D in enumerate(WIDTHS):
        B = [1, 37, 1000, 4099][ci % 4]
        case = "obs %d rows=%d" % (D, B)
        rs = np.random.RandomState(3000 + ci)
        cs = TO.critic_spec(D)
        tc = TO.draw_tower(cs, rs)
        obs = rs.randn(B, D).astype(np.float32)
        got = torch.full((B,), np.nan, device=DEV)
        ops.critic_values(ops.net_desc(D, 1, ops.HEAD_VALUE), dev(tc), dev(obs), got)
        torch.cuda.synchronize()
        _check_values(led, case, got.cpu().numpy(), cs, tc, obs)
    led.assert_ok()
    cs = TO.critic_spec(257)
    with pytest.raises(ops.nat.NativeError, match="obs_dim 257"):
        ops.critic_values(ops.net_desc(257, 1, ops.HEAD_VALUE), dev(torch.zeros(cs.n_params())), dev(np.zeros((3, 257))),
                          torch.empty(3, device=DEV))
    with pytest.raises(ops.nat.NativeError, match="obs_dim 257"):
        ops.act_step(ops.net_desc(257, 2, ops.HEAD_CATEGORICAL), dev(torch.zeros(TO.spec(257, "disc", 2).n_params())),
                     None, None, dev(np.zeros((3, 257))), None, None, 3, True, 0, 0, 0, None, None,
                     torch.empty(3, 1, device=DEV), torch.empty(3, 1, device=DEV))
    got = torch.full((5,), np.nan, device=DEV)
    rs = np.random.RandomState(7)
    cs = TO.critic_spec(256)
    tc, obs = TO.draw_tower(cs, rs), rs.randn(5, 256).astype(np.float32)
    ops.critic_values(ops.net_desc(256, 1, ops.HEAD_VALUE), dev(tc), dev(obs), got)
    led = TO.Ledger(ATOL, RTOL, K)
    _check_values(led, "obs 256 after a refusal", got.cpu().numpy(), cs, tc, obs)
    led.assert_ok()


# ------------------------------------------------------------------------------------------------ fused rollout
ROLL_WIDTHS = [1, 4, 8, 9, 17, 33, 64, 65, 68, 69, 100, 152, 156]
ROLL_HEADS = [("disc", 2, False), ("disc", 9, True), ("box", 1, False), ("box", 6, False)]
LOCKSTEP_MAX = {False: 156, True: 152}  # by "more than 2 outputs": the lock-step kernel's LDS fit


class _Rollout:
    """Buffers of one single-agent synthetic-env rollout [T+1, N, 1, .] (the layout of NormalReplayBuffer), filled by
    orl_env_reset; launch() runs orl_rollout_fused on them and next() moves slot T to slot 0 like after_update."""

    def __init__(self, ops, D, n, head_kind, K_mask, N, T, limit, env_seed):
        self.ops, self.D, self.N, self.T, self.limit, self.env_seed = ops, D, N, T, limit, env_seed
        a_w = 1 if head_kind == ops.HEAD_CATEGORICAL else n
        z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=DEV)
        o = lambda *s: torch.ones(*s, dtype=torch.float32, device=DEV)
        self.obs = z(T + 1, N, 1, D)
        self.rewards, self.masks, self.bad, self.active = z(T, N, 1, 1), o(T + 1, N, 1, 1), o(T + 1, N, 1, 1), o(T + 1, N, 1, 1)
        self.amask = z(T + 1, N, 1, K_mask) if K_mask else None
        self.K = K_mask
        self.value_preds, self.next_value = torch.full((T + 1, N, 1, 1), np.nan, device=DEV), torch.full((N,), np.nan, device=DEV)
        self.actions, self.logp = z(T, N, 1, a_w), z(T, N, 1, a_w)
        self.env_state = z(N, ops.env_state_width(ops.ENV_SYNTH))
        self.ep_stats = z(N, 4)
        ops.env_reset(ops.ENV_SYNTH, self.env_state, self.ep_stats, self.obs[0], N, D, env_seed, limit)
        self.step0 = 0

    def launch(self, pnet, tp, cnet, tc, act_seed, kernel):
        nat, f = self.ops.nat, self.ops.nat.fptr
        buf = nat.BufferPtrs(f(self.obs), f(self.obs), f(self.rewards), f(self.masks), f(self.bad), f(self.active),
                             f(self.amask), self.T, self.N, 1, self.D, self.D, self.K)
        args = nat.RolloutArgs(buf, f(self.value_preds), f(self.actions), f(self.logp), f(self.env_state), f(self.ep_stats),
                               self.ops.ENV_SYNTH, self.limit, self.env_seed, act_seed, self.step0)
        args.opp_reserved = 1 if kernel == "lockstep" else 0
        self.ops.rollout_fused(pnet, tp, cnet, tc, args, self.next_value)

    def fetch(self):
        torch.cuda.synchronize()
        return {k: getattr(self, k).cpu().numpy().copy() for k in
                ("obs", "rewards", "masks", "value_preds", "next_value", "actions", "logp")} | (
                   {"amask": self.amask.cpu().numpy().copy()} if self.amask is not None else {})

    def next(self):
        for t in (self.obs, self.masks, self.bad, self.active) + ((self.amask,) if self.amask is not None else ()):
            t[0].copy_(t[-1])
        self.value_preds.fill_(np.nan)
        self.next_value.fill_(np.nan)
        self.step0 += self.T


def _check_rollout(led, case, r, orc, ps, cs, tp, tc, act_seed, step0):
    """One launch's buffers against the env oracle (continuing from its state) and the float64 towers on the stored
    observations."""
    T, N = r["actions"].shape[:2]
    n = ps.n_out
    rows = np.arange(N)
    obs = r["obs"][:, :, 0]
    for t in range(T):
        oo, rr, dd, _ = orc.step()
        if not np.allclose(obs[t + 1], oo[:, 0], rtol=1e-5, atol=2e-6):
            led.fail("%s t=%d: stored observations are not the synthetic env's stream (max diff %.3g)" % (
                case, t, np.abs(obs[t + 1] - oo[:, 0]).max()))
        if not np.array_equal(r["rewards"][t], rr):
            led.fail("%s t=%d: rewards differ from the env oracle" % (case, t))
        if not np.array_equal(r["masks"][t + 1, :, :, 0], np.where(dd, 0.0, 1.0).astype(np.float32)):
            led.fail("%s t=%d: masks differ from the env oracle's done schedule" % (case, t))
    if "amask" in r and not np.all(r["amask"][1:] == 1.0):
        led.fail("%s: the synthetic env's action masks are not all ones" % case)
    x = obs.reshape(-1, ps.obs_dim)                       # all T+1 slots
    v64 = TO.head_fields(cs, tc, x, torch.float64)["out"].reshape(T + 1, N)
    v32 = TO.head_fields(cs, tc, x, torch.float32)["out"].reshape(T + 1, N)
    b = led.check(case, "value", r["value_preds"][:T, :, 0, 0], v64[:T], v32[:T])
    led.check(case, "next_value", r["next_value"], v64[T], v32[T])
    # slot T: the chain kernel writes the bootstrap value there too, the lock-step kernel leaves it to compute_returns
    vT = r["value_preds"][T, :, 0, 0]
    if not (np.isnan(vT).all() or np.array_equal(vT, r["next_value"])):
        led.fail("%s: value_preds[T] is neither untouched nor next_value" % case)
    TO.check_sensitivity(led, case, "value", TO.tail_sensitivity(cs, tc, x).reshape(T + 1, N)[:T], b)
    for t in range(T):
        tg = step0 + t
        c = "%s t=%d" % (case, t)
        if ps.head == po.HEAD_CATEGORICAL:
            u = TO.philox_uniforms(act_seed, rows, tg)
            f64 = TO.head_fields(ps, tp, obs[t], torch.float64)
            f32 = TO.head_fields(ps, tp, obs[t], torch.float32)
            a = r["actions"][t, :, 0, 0]
            ok = TO.sample_edge_ok(a, u, f64["out"], None, CDF_TOL)
            if not ok.all():
                led.fail("%s: %d of %d sampled actions are not the float64 sample" % (c, int((~ok).sum()), N))
                continue
            ai = a.astype(np.int64)
            led.check(c, "logp", r["logp"][t, :, 0, 0], f64["logp_all"][rows, ai], f32["logp_all"][rows, ai])
        else:
            eps = TO.philox_normals(act_seed, rows, tg, n)
            f64 = TO.head_fields(ps, tp, obs[t], torch.float64, eps=eps)
            f32 = TO.head_fields(ps, tp, obs[t], torch.float32, eps=eps.astype(np.float32))
            led.check(c, "action", r["actions"][t, :, 0], f64["act"], f32["act"])
            led.check(c, "logp", r["logp"][t, :, 0], f64["logp"], f32["logp"])
        if t == 0:
            TO.check_sensitivity(led, c, "head", TO.tail_sensitivity(ps, tp, obs[t]),
                                 TO.bar(f64["out"], f32["out"], ATOL, RTOL, K))


@pytest.mark.parametrize("kernel", ["chain", "lockstep"])
def test_fused_rollout_teacher_forced_across_the_envelope(ops, kernel):
    """orl_rollout_fused on the synthetic env, N = 70 (4 full 16-row tiles + a ragged one), T = 12 (past the chain kernel's
    8-slot observation ring and its 3 critic waves), two launches (the second from the first one's env state): every step's
    values, next_value, actions and log-probs against float64 on the stored observations, Philox uniforms / normals of the
    kernel's counters, and the env stream against SynthEnvOracle (rewards and masks bit-exact; observations to the
    transcendental round-off of the oracle's float32 Box-Muller).  value_preds[0..T-1] and next_value are checked; slot T
  holds next_value (chain kernel) or is left to compute_returns (lock-step kernel).  ``chain`` is opp_reserved = 0 (the default: the chain
    kernel up to obs 64, the lock-step kernel above), ``lockstep`` opp_reserved = 1.  Widths past the lock-step kernel's
    LDS fit are refused with a message, and the next launch works."""
    N, T, limit = 70, 12, 5
    led = TO.Ledger(ATOL, RTOL, K)
    ci = 0
    for D in ROLL_WIDTHS:
        for head in ROLL_HEADS:
            h, n, m = head
            if D > LOCKSTEP_MAX[n > 2]:
                continue
            ci += 1
            case = "%s %s" % (kernel, _name(D, head))
            rs = np.random.RandomState(4000 + 97 * D + ci)
            ps, cs = TO.spec(D, h, n), TO.critic_spec(D)
            tp, tc = TO.draw_tower(ps, rs), TO.draw_tower(cs, rs)
            pnet, cnet = ops.net_desc(D, n, ps.head), ops.net_desc(D, 1, ops.HEAD_VALUE)
            env_seed, act_seed = 11 + ci, 100003 * ci + 5
            ro = _Rollout(ops, D, n, ps.head, n if m else 0, N, T, limit, env_seed)
            orc = po.SynthEnvOracle(N, D, env_seed, limit)
            o0 = ro.obs[0, :, 0].cpu().numpy()
            if not np.allclose(o0, orc.reset()[:, 0], rtol=1e-5, atol=2e-6):
                led.fail("%s: reset observations are not the synthetic env's" % case)
            for launch in range(2):
                ro.launch(pnet, dev(tp), cnet, dev(tc), act_seed, kernel)
                _check_rollout(led, "%s launch %d" % (case, launch), ro.fetch(), orc, ps, cs, tp, tc, act_seed, ro.step0)
                ro.next()
    # the refusal boundary: one column past the lock-step kernel's LDS fit, per head width
    for head, D in ((("disc", 2, False), 157), (("disc", 9, True), 153), (("box", 6, False), 153)):
        h, n, m = head
        ps, cs = TO.spec(D, h, n), TO.critic_spec(D)
        ro = _Rollout(ops, D, n, ps.head, n if m else 0, N, T, limit, 1)
        with pytest.raises(ops.nat.NativeError, match="LDS"):
            ro.launch(ops.net_desc(D, n, ps.head), dev(torch.zeros(ps.n_params())), ops.net_desc(D, 1, ops.HEAD_VALUE),
                      dev(torch.zeros(cs.n_params())), 1, kernel)
        D -= 1  # the widest width admitted: runs
        rs = np.random.RandomState(D)
        ps, cs = TO.spec(D, h, n), TO.critic_spec(D)
        tp, tc = TO.draw_tower(ps, rs), TO.draw_tower(cs, rs)
        ro = _Rollout(ops, D, n, ps.head, n if m else 0, N, T, limit, 3)
        orc = po.SynthEnvOracle(N, D, 3, limit)
        orc.reset()
        ro.launch(ops.net_desc(D, n, ps.head), dev(tp), ops.net_desc(D, 1, ops.HEAD_VALUE), dev(tc), 9, kernel)
        _check_rollout(led, "%s %s after a refusal" % (kernel, _name(D, head)), ro.fetch(), orc, ps, cs, tp, tc, 9, 0)
    led.assert_ok()


# ------------------------------------------------------------------------------------------------ routing past 64
def test_observations_wider_than_64_train_on_the_general_towers():
    """The default towers' update kernels take obs <= 64 (orl_ppo.hip / orl_rnn.hip check_net), so PPOModule routes a wider
    observation to the general towers: SyntheticFixedStep-v0 at obs 100 trains through make / PPONet / PPOAgent.train on
    GenericPPOModule with the fused general rollout, and one full-batch update's gradients match po.ppo_update (the check
    of test_single_update_at_baseline_shapes_vs_oracle, at this shape)."""
    from openrl_amd import spaces
    from openrl_amd.configs.config import default_cfg
    from openrl_amd.envs.common import make
    from openrl_amd.modules.common import PPONet
    from openrl_amd.modules.generic_net import GenericPPOModule
    from openrl_amd.runners.common import PPOAgent
    from tests.test_ppo_update_gpu import _random_case

    cfg = default_cfg(["--episode_length", "12", "--ppo_epoch", "2"])
    env = make("SyntheticFixedStep-v0", env_num=40, obs_dim=100, action_space=spaces.Discrete(3), episode_limit=5,
               device=DEV)
    agent = PPOAgent(PPONet(env, cfg=cfg, device=DEV))
    assert isinstance(agent.net.module, GenericPPOModule)
    agent.train(total_time_steps=40 * 12 * 3)
    assert agent.driver.fused and agent.driver.fused_generic and agent.num_time_steps == 40 * 12 * 3
    d = agent.driver.buffer.data
    assert torch.isfinite(d.returns).all() and torch.isfinite(d.action_log_probs).all()
    assert d.actions.min() >= 0 and d.actions.max() <= 2 and len(torch.unique(d.actions)) > 1

    D, n_act = 100, 3
    cfg, module, buf, algo, host, a_w = _random_case(D, "discrete", n_act, 40, 9, seed=D, masks=True)
    assert isinstance(module, GenericPPOModule)
    hp = po.hyper_from_cfg(cfg)
    pspec, cspec = po.TowerSpec(D, n_act, po.HEAD_CATEGORICAL), po.TowerSpec(D, 1, po.HEAD_VALUE)
    ptheta = module.models["policy"].reference_flat().cpu().clone()
    ctheta = module.models["critic"].reference_flat().cpu().clone()
    assert ptheta.numel() == pspec.n_params() and ctheta.numel() == cspec.n_params()
    padam, cadam = po.AdamOracle(ptheta.numel(), cfg.lr), po.AdamOracle(ctheta.numel(), cfg.critic_lr)
    vn = po.ValueNormOracle()
    adv = po.advantages(host["returns"], host["value_preds"], host["active_masks"], vn, False)
    fr = po.flat_rows
    sample = (fr(host["critic_obs"][:-1]), fr(host["policy_obs"][:-1]), fr(host["actions"]),
              fr(host["value_preds"][:-1]), fr(host["returns"][:-1]), fr(host["active_masks"][:-1]),
              fr(host["action_log_probs"]), adv.reshape(-1, 1), fr(host["action_masks"][:-1]))
    _, gp, gc = po.ppo_update(hp, pspec, ptheta, cspec, ctheta, padam, cadam, vn, sample)
    algo._advantages_and_records(buf)
    algo._info.zero_()
    algo._update_minibatch(buf, None, adv.size, True)
    torch.cuda.synchronize()
    got_p = module.models["policy"].reference_grad_flat().cpu().numpy()
    got_c = module.models["critic"].reference_grad_flat().cpu().numpy()
    np.testing.assert_allclose(got_p, gp, rtol=2e-3, atol=3e-5 * np.abs(gp).max() + 1e-7)
    np.testing.assert_allclose(got_c, gc, rtol=2e-3, atol=3e-5 * np.abs(gc).max() + 1e-7)

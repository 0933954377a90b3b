"""Helpers of the shared-filter IQN trainer's tests (not collected).

* ``SharedIQNEmulator``: ``shared_cases.SharedEmulator`` plus ``tg_iqn_head_fwd`` / ``tg_iqn_head_bwd`` written out from the
  header's formulas in plain torch, in the dtype of their arguments (fp32 in the tests).
* ``head_ref``: the head behind the pooled features restated in differentiable torch ops (any dtype; the tests use float64).
* ``head_case``: inputs of one head case, the float64 truth of every output of both entry points and of the double backward
  (autograd of ``head_ref``), and ``e32``, the error the same ATen ops make in float32 on the CPU, for each choice of cotangent
  parts (``variants``); ``limit`` is shared_cases'.
* ``shared_iqn_trainer`` / ``load_shared_iqn_fixture`` / ``load_procedural``: the trainer a ``tests/golden/shared_iqn_*.json``
  fixture describes."""
import functools
import json
import math
import os

import torch
import torch.nn.functional as F

from shared_cases import GOLDEN_DIR, SharedEmulator, limit, shared_config, shared_state  # noqa: F401

SHARED_IQN_CASES = ('shared_iqn_c16_b4', 'shared_iqn_c32a2_b4', 'shared_iqn_c32_b2_id')
OUTPUTS_FWD = ('pt', 'loss', 'dpreds')
OUTPUTS_BWD = ('df', 'dW1', 'db1', 'dw2', 'db2')
OUTPUTS_DBWD = ('d_gpt', 'd_W1', 'd_b1', 'd_w2')


# ------------------------------------------------------------------------------------------------------------- emulator
def _rows(f, G, B, Q, C):
    """(G*B, C) -> (G*Q*B, C), row g*Q*B + q*B + b"""
    return f.reshape(G, 1, B, C).expand(G, Q, B, C).reshape(G * Q * B, C)


def _embed(taus, rng, R, D):
    return torch.cos((taus.reshape(R, 1) * math.pi) * rng.reshape(1, D))


def _huber_terms(p, t, taus, k, G, B, Q):
    """-> (weight * huber, d loss / d p) per row, both (G, Q, B)"""
    err = t.reshape(G, 1, B) - p.reshape(G, Q, B)
    a = err.abs()
    hub = torch.where(a <= k, 0.5 * err * err, k * (a - 0.5 * k))
    dh = torch.where(a <= k, err, k * torch.sign(err))
    wgt = (taus.reshape(G, Q, B) - (err < 0).to(p.dtype)).abs()
    return wgt * hub, -wgt * dh / B


class SharedIQNEmulator(SharedEmulator):
    def iqn_head_workspace(self, G, B):
        return 8 * G * B

    def iqn_head_fwd(self, f, taus, target, W1, b1, w2, b2, rng, k, pt, loss, dpreds, ws, G, B, Q, C, D):
        R = G * Q * B
        s = torch.tanh(_embed(taus, rng, R, D) @ W1.reshape(C, D).t() + b1.reshape(1, C))
        p = (_rows(f, G, B, Q, C) * s) @ w2.reshape(C) + (b2.reshape(()) if b2 is not None else 0.)
        pt.view(-1).copy_(p.reshape(G, Q, B).sum(1).reshape(-1) / Q)
        if target is not None:
            terms, dp = _huber_terms(p, target, taus, k, G, B, Q)
            loss.copy_(terms.sum(1).mean(-1).sum())
            dpreds.view(-1).copy_(dp.reshape(-1))
        return 0

    def iqn_head_bwd(self, gl, gpt, dpreds, f, taus, W1, b1, w2, rng, df, dW1, db1, dw2, db2, G, B, Q, C, D, accumulate):
        R = G * Q * B
        e = _embed(taus, rng, R, D)
        s = torch.tanh(e @ W1.reshape(C, D).t() + b1.reshape(1, C))
        delta = torch.zeros(R, dtype=f.dtype)
        if gl is not None:
            delta = delta + gl.reshape(()) * dpreds.reshape(R)
        if gpt is not None:
            delta = delta + (gpt.reshape(G, 1, B) / Q).expand(G, Q, B).reshape(R)
        fr, wv = _rows(f, G, B, Q, C), w2.reshape(1, C)
        ds = delta.reshape(R, 1) * s
        da = delta.reshape(R, 1) * fr * wv * (1 - s * s)

        def put(out, value):
            if out is not None:
                out.copy_((out + value.reshape(out.shape)) if accumulate else value.reshape(out.shape))
        if df is not None:
            df.copy_((wv * ds.reshape(G, Q, B, C).sum(1).reshape(G * B, C)).reshape(df.shape))
        put(dw2, (ds * fr).sum(0))
        put(db2, delta.sum())
        put(dW1, da.t() @ e)
        put(db1, da.sum(0))
        return 0


# ------------------------------------------------------------------------------------------------- the float64 restatement
def head_ref(f, taus, W1, b1, w2, b2, rng, G, B, Q):
    """-> p (G*Q*B), pt (G*B): cos embedding -> Linear -> tanh -> * repeated features -> Linear, and the quantile mean."""
    R, C = G * Q * B, f.shape[1]
    e = torch.cos((taus.reshape(R, 1) * math.pi) * rng)
    s = torch.tanh(F.linear(e, W1, b1))
    p = F.linear(_rows(f, G, B, Q, C) * s, w2.reshape(1, C), b2).reshape(R)
    return p, p.reshape(G, Q, B).mean(1).reshape(G * B)


def head_loss(p, t, taus, k, G, B, Q):
    """models/iqn.py:111-130 per evaluation, summed over the G evaluations."""
    err = t.reshape(G, 1, B) - p.reshape(G, Q, B)
    a = err.abs()
    hub = torch.where(a <= k, 0.5 * err.pow(2), k * (a - 0.5 * k))
    wgt = (taus.reshape(G, Q, B) - (err.detach() < 0).to(p.dtype)).abs()
    return (wgt * hub).sum(1).mean(-1).sum()


def _rel(got, want):
    scale = float(want.abs().max())
    return float((got - want).abs().max()) / scale if scale > 0 else float((got - want).abs().max())


def head_outputs(c, dtype, use_gl=True, use_gpt=True):
    """Every output of both entry points and of the double backward, by autograd of ``head_ref`` in ``dtype`` -> dict of float64."""
    G, B, Q, k = c['G'], c['B'], c['Q'], c['k']
    f, W1, b1, w2, b2 = (c[n].to(dtype).clone().requires_grad_(True) for n in ('f', 'W1', 'b1', 'w2', 'b2'))
    gpt = c['gpt'].to(dtype).clone().requires_grad_(True)
    taus, t, rng, gl, v = (c[n].to(dtype) for n in ('taus', 't', 'range', 'gl', 'v'))
    p, pt = head_ref(f, taus, W1, b1, w2, b2, rng, G, B, Q)
    loss = head_loss(p, t, taus, k, G, B, Q)
    dpreds, = torch.autograd.grad(loss, p, retain_graph=True)
    delta = torch.zeros_like(p)
    if use_gl:
        delta = delta + gl * dpreds              # (dpreds: a constant of the second order)
    if use_gpt:
        delta = delta + (gpt.reshape(G, 1, B) / Q).expand(G, Q, B).reshape(-1)
    psi = (delta * p).sum()
    df, dW1, db1, dw2, db2 = torch.autograd.grad(psi, (f, W1, b1, w2, b2), create_graph=True)
    out = dict(pt=pt, loss=loss.reshape(1), dpreds=dpreds, df=df, dW1=dW1, db1=db1, dw2=dw2.reshape(-1), db2=db2)
    second = torch.autograd.grad((v * df).sum(), (gpt, W1, b1, w2), allow_unused=True)
    for name, g, like in zip(OUTPUTS_DBWD, second, (gpt, W1, b1, w2)):
        out[name] = (torch.zeros_like(like) if g is None else g).reshape(-1)
    return {n: x.detach().double() for n, x in out.items()}


@functools.lru_cache(maxsize=None)
def head_case(G, B, Q, C, D, k=1.0, seed=0):
    """One head case, computed once: inputs (fp32), ``want`` (float64 truth per output, with both cotangent parts) and ``e32``.
    Features are sums over a plane of activations (scale 4); W1 / w2 are Linear-sized; targets 0 / 1 like the trainer's labels,
    so that rows fall on both sides of the Huber threshold."""
    gen = torch.Generator().manual_seed(100003 * seed + 10007 * G + 1009 * B + 101 * Q + 11 * C + D)
    rn = lambda *shape: torch.randn(*shape, generator=gen)
    c = dict(G=G, B=B, Q=Q, C=C, D=D, k=k, f=rn(G * B, C) * 4, taus=torch.rand(G * Q * B, generator=gen),
             t=(torch.rand(G * B, generator=gen) < 0.5).float(), W1=rn(C, D) * D ** -0.5, b1=rn(C) * 0.1, w2=rn(1, C) * C ** -0.5,
             b2=rn(1) * 0.1, range=torch.arange(1, D + 1).float(), gl=rn(()).abs() + 0.5, gpt=rn(G * B), v=rn(G * B, C))
    c['variants'] = {}
    for use_gl, use_gpt in ((True, True), (True, False), (False, True)):          # which parts of the cotangent are given
        want, r32 = head_outputs(c, torch.float64, use_gl, use_gpt), head_outputs(c, torch.float32, use_gl, use_gpt)
        c['variants'][use_gl, use_gpt] = (want, {n: _rel(r32[n], want[n]) for n in want})
    c['want'], c['e32'] = c['variants'][True, True]
    return c


# -------------------------------------------------------------------------------------------------------------- fixtures
def load_shared_iqn_fixture(name):
    with open(os.path.join(GOLDEN_DIR, name + '.json')) as f:
        return json.load(f)


def shared_iqn_trainer(fx, device, seed=0, cls=None, **overrides):
    from tartangan_amd.trainers.shared.iqn import IQNTrainer
    cls = cls or IQNTrainer
    tr = cls(cls.default_args(config=shared_config(fx), batch_size=fx['batch'], device=device, **{**fx['flags'], **overrides}))
    torch.manual_seed(seed)
    tr.build_models()
    return tr


def load_procedural(tr, fx):
    tr.g.load_state_dict(shared_state(tr.g.state_dict(), fx['weight_seed']))
    tr.target_g.load_state_dict(shared_state(tr.target_g.state_dict(), fx['weight_seed'] + 1))
    tr.d.load_state_dict(shared_state(tr.d.state_dict(), fx['weight_seed'] + 2))


def total_l2(module, grads=False):
    s = 0.
    for p in module.parameters():
        t = p.grad if grads else p
        if t is not None:
            s += float(t.detach().double().pow(2).sum())
    return s ** 0.5

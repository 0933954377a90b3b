"""The per-op first- and second-order harness (tests/second_order_cases.py) on the HIP kernels: every op on the
discriminator's path (and the generator-phase ops at first order) against stock torch in float64, with the pass rule "no
worse than plain fp32 on the CPU".  Ragged small shapes and the exact edges run in process at the default convolution
dispatch and again, for the convolution family, in child processes with TG_CONV_WINO=0 (direct kernels only) and =2
(Winograd on every eligible shape): the knob is read once per process.  The discriminator's own layer shapes (recorded
from the D phase of one training step at batch 64, whose real | fake pair runs at 128) run at the default dispatch."""
import os
import subprocess
import sys

import pytest
import torch

import second_order_cases as SO

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = SO.ragged_cases() + SO.edge_cases()
CONV_KINDS = ('conv2d_3x3', 'conv2d_1x1', 'compose_rgb', 'pool_conv3x3', 'upconv3x3')


def _report(case, errs):
    """One line per case: the worst e_op / e_32 of each level (what the pass rule bounds by 4)."""
    worst = {}
    for k, (e, e32, *_rest) in errs.items():
        lvl = k.split('.')[0]
        worst[lvl] = max(worst.get(lvl, 0.0), e / max(e32, SO.EPS))
    mode = os.environ.get('TG_CONV_WINO', 'default')
    print(f'SO_TABLE wino={mode} {case.name} ' + ' '.join(f'{k}={v:.2f}' for k, v in sorted(worst.items())))


@pytest.mark.parametrize('case', CASES, ids=[c.name for c in CASES])
def test_op_matches_float64_torch_to_first_and_second_order(case):
    errs, bad = SO.run_case(case, 'cuda')
    torch.cuda.synchronize()
    _report(case, errs)
    assert not bad, bad


@pytest.mark.parametrize('mode', ['0', '2'])
def test_convolution_cases_under_each_winograd_mode(mode):
    env = dict(os.environ, TG_CONV_WINO=mode)
    sel = 'test_op_matches_float64_torch_to_first_and_second_order and (' + ' or '.join(CONV_KINDS) + ')'
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-q', '-s', '-k', sel, '-p', 'no:cacheprovider'],
                       env=env, cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    print('\n'.join(line[line.index('SO_TABLE'):] for line in r.stdout.splitlines() if 'SO_TABLE' in line))
    assert r.returncode == 0, r.stdout[-4000:]
    assert ' passed' in r.stdout and ' deselected' in r.stdout


def _d_phase_launches(config, batch=64, kind='iqn'):
    """Launch shapes of the D phase of one training step (the generator's forward inside it excluded)."""
    from tartangan_amd import backend
    from tartangan_amd.models.pluggan import GAN_CONFIGS
    from tartangan_amd.trainers.cnn import CNNTrainer
    from tartangan_amd.trainers.iqn import IQNTrainer
    name, att = config.split(':')
    cfg = GAN_CONFIGS[name]._replace(attention=(int(att),))
    cls = {'cnn': CNNTrainer, 'iqn': IQNTrainer}[kind]
    tr = cls(cls.default_args(config=cfg, batch_size=batch, device='cuda'))
    torch.manual_seed(1234)
    tr.build_models()
    K = backend.get()
    rec = SO.Recorder(K, SO.D_ENTRY_POINTS)
    gen_fwd, d_phase = tr._generator_forward_for_both_phases, tr._d_phase

    def quiet_generator(*a, **kw):
        rec.__exit__(None, None, None)
        try:
            return gen_fwd(*a, **kw)
        finally:
            rec.__enter__()

    def recorded_d_phase(*a, **kw):
        with rec:
            return d_phase(*a, **kw)
    tr._generator_forward_for_both_phases, tr._d_phase = quiet_generator, recorded_d_phase
    size = int(name)
    g = torch.Generator().manual_seed(7)
    tr.train_batch((torch.rand(batch, 3, size, size, generator=g) * 2 - 1).cuda())
    torch.cuda.synchronize()
    return rec.seen


@pytest.mark.parametrize('config', ['64:1', '128:3'])
def test_discriminator_layer_shapes_match_float64_torch(config):
    seen = _d_phase_launches(config)
    cases = SO.cases_from_launches(seen)
    kinds = {c.kind for c in cases}
    assert {'conv2d_3x3', 'pool_conv3x3', 'attention_core', 'batch_norm_act'} <= kinds, sorted(kinds)
    failures = []
    for case in cases:
        errs, bad = SO.run_case(case, 'cuda')
        torch.cuda.synchronize()
        _report(case, errs)
        failures += [f'{case.name}: {b}' for b in bad]
    assert not failures, failures


# --------------------------------------------------------------------------- the D phase against a float64 oracle
D_PHASE_CASES = ['c32a2_iqn_b8', 'c64a1_cnn_b8', 'c64a1_iqn_b8', 'c128a3_cnn_b4', 'c32_cnn_b8_selu', 'c32_cnn_b8_elu', 'c64a1_iqn_b64']
D_PHASE_SEEDS = range(5)


def _d_phase_inputs(fx, seed):
    """(real, fake, (taus of D(real), taus of D(fake)) or None): the same batch for the HIP trainer and both oracles."""
    from oracle.procedural import synthetic_images
    B, size = fx['batch'], fx['size']
    real = synthetic_images(B, size, fx['img_seed'] + seed)
    fake = synthetic_images(B, size, fx['img_seed'] + 1000 + seed)
    taus = None
    if fx['trainer'] == 'iqn':
        from oracle import sagan_cpu as O
        g = torch.Generator().manual_seed(5000 + seed)
        taus = tuple(torch.rand(B * O.NUM_QUANTILES, 1, generator=g) for _ in range(2))
    return real, fake, taus


def _oracle(fx):
    from oracle import sagan_cpu as O
    from oracle.procedural import procedural_state
    torch.manual_seed(0)
    ref = O.OracleTrainer(fx['config'], fx['trainer'], fx['batch'], attention=fx['attention'], **fx.get('flags', {}))
    ref.load(d=procedural_state(ref.d, fx['weight_seed'] + 2))
    return ref


_ORACLE_RUNS = {}


def oracle_d_phase(fx, seed, dtype, buffers=None):
    """oracle/sagan_cpu.py OracleTrainer.train_batch's D phase (up to d_loss.backward()) on the state cast to ``dtype``:
    the losses and every parameter gradient.  ``buffers``: a key prefix under which D's BatchNorm buffers after the phase (the
    oracle updates them in place: the real pass, then the fake pass) are returned as well -- running statistics as float64,
    num_batches_tracked as it is.  A (fixture, seed, dtype) is computed once per process."""
    import json
    key = (json.dumps(fx, sort_keys=True), seed, dtype)
    if key not in _ORACLE_RUNS:
        _ORACLE_RUNS[key] = _oracle_d_phase(fx, seed, dtype)
    out, bufs = _ORACLE_RUNS[key]
    out = dict(out)
    if buffers is not None:
        out.update({buffers + k: v for k, v in bufs.items()})
    return out


def _oracle_d_phase(fx, seed, dtype):
    from oracle import sagan_cpu as O
    ref = _oracle(fx)                                        # (sets the oracle's activation option for this case)
    S = {}
    for k, v in ref.d.items():
        v = v.detach().to(dtype) if v.is_floating_point() else v.detach().clone()
        S[k] = v.requires_grad_() if O.is_param(k) else v
    real, fake, taus = _d_phase_inputs(fx, seed)
    real, fake = real.to(dtype).requires_grad_(), fake.to(dtype)
    B = fx['batch']
    labels = torch.zeros(2 * B, 1, dtype=dtype)
    labels[:B] = 1
    if fx['trainer'] == 'iqn':
        p_real, l_real = O.iqn_d_forward(S, real, ref.cfg, targets=labels[:B], taus=taus[0].to(dtype))
        _, l_fake = O.iqn_d_forward(S, fake, ref.cfg, targets=labels[B:], taus=taus[1].to(dtype))
        d_loss = l_real + l_fake
    else:
        p_real = O.d_forward(S, real, ref.cfg)
        d_loss = torch.nn.functional.binary_cross_entropy_with_logits(torch.cat([p_real, O.d_forward(S, fake, ref.cfg)], 0), labels)
    gp = ref.grad_penalty * O.gradient_penalty(p_real, real)
    d_loss = d_loss + gp
    d_loss.backward()
    out = {'d_loss': d_loss.detach(), 'gp': gp.detach()}
    out.update({k: v.grad for k, v in S.items() if O.is_param(k) and v.grad is not None})
    bufs = {k: (v.to(torch.float64) if v.is_floating_point() else v.clone()) for k, v in S.items()
            if 'running_' in k or 'num_batches_tracked' in k}
    return {k: v.to(torch.float64) for k, v in out.items()}, bufs


def hip_d_phase(fx, seed):
    """The HIP trainer's ``_d_phase`` (gradients before the optimiser step) from the same un-stepped state and inputs."""
    from conftest import trainer_from_fixture
    ref = _oracle(fx)
    tr = trainer_from_fixture(fx, 'cuda')
    tr.d.load_state_dict({k: v.clone() for k, v in ref.d.items()})
    real, fake, taus = _d_phase_inputs(fx, seed)
    fake = fake.cuda()
    tr._generator_forward_for_both_phases = lambda bs: None
    tr.sample_g = lambda n=None, **kw: fake
    if taus is not None:
        feed = [t.cuda() for t in taus]
        heads = [m for m in tr.d.modules() if hasattr(m, 'tau_source')]
        assert len(heads) == 1
        heads[0].tau_source = lambda rows, nq: feed.pop(0)
    tr._training_mode()
    d_loss, gp = tr._d_phase(real.cuda())
    if taus is not None:
        assert not feed, 'the D phase did not draw both tau sets'
    out = {'d_loss': d_loss, 'gp': gp}
    out.update({k: p.grad for k, p in tr.d.named_parameters() if p.grad is not None})
    return {k: v.detach().to('cpu', torch.float64) for k, v in out.items()}


def _hip_child(cases, seeds, mode, path):
    """The HIP D phases in a child process with TG_CONV_WINO=mode (read once per process), written to ``path``."""
    code = ('import sys, torch; sys.path[:0] = [%r, %r]; import test_second_order_gpu as T; '
            'torch.save({c: [T.hip_d_phase(T.load_golden(c), s) for s in %r] for c in %r}, %r)'
            % (os.path.join(REPO, 'tests'), REPO, list(seeds), list(cases), str(path)))
    r = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, TG_CONV_WINO=mode), cwd=REPO, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    return torch.load(path)


def load_golden(case):
    from conftest import load_golden as load
    return load(case)


def d_phase_ratios(cases, seeds, modes, tmp_path):
    """-> {(mode, case): {quantity: (median e_hip, median e_32)}} over the seeds; CPU references computed once, here."""
    refs = {c: [(oracle_d_phase(load_golden(c), s, torch.float64), oracle_d_phase(load_golden(c), s, torch.float32))
                for s in seeds] for c in cases}
    out = {}
    for mode in modes:
        got = _hip_child(cases, seeds, mode, tmp_path / f'd_phase_wino{mode}.pt')
        for c in cases:
            per = {}
            for (r64, r32), hip in zip(refs[c], got[c]):
                assert set(hip) == set(r64), sorted(set(hip) ^ set(r64))
                for k, T64 in r64.items():
                    n = float(T64.norm()) or 1.0
                    per.setdefault(k, []).append((float((hip[k] - T64).norm()) / n, float((r32[k] - T64).norm()) / n))
            out[(mode, c)] = {k: (sorted(e for e, _ in v)[len(v) // 2], sorted(e for _, e in v)[len(v) // 2]) for k, v in per.items()}
    return out


def test_d_phase_r1_gradients_match_float64_oracle(tmp_path):
    """d_loss, gp and every D parameter gradient of one D phase (R1 penalty included) from un-stepped procedural state:
    HIP against the oracle in float64, next to the same oracle in fp32.  Mask flips cannot be avoided at this size, so the rule
    is on the median over 5 image seeds: median e_hip <= 4 median e_32, for both convolution kernel families."""
    failures = []
    for (mode, case), stats in d_phase_ratios(D_PHASE_CASES, D_PHASE_SEEDS, ('0', '2'), tmp_path).items():
        worst = max(stats, key=lambda k: stats[k][0] / max(stats[k][1], SO.EPS))
        e, e32 = stats[worst]
        print(f'DPHASE wino={mode} {case} worst={worst} ratio={e / max(e32, SO.EPS):.2f} gp={stats["gp"][0]:.2e}/{stats["gp"][1]:.2e} '
              f'd_loss={stats["d_loss"][0]:.2e}/{stats["d_loss"][1]:.2e}')
        failures += [f'wino={mode} {case} {k}: median e_hip {a:.2e} e_32 {b:.2e}' for k, (a, b) in stats.items()
                     if a > SO.RATIO_L2 * max(b, SO.EPS)]
    assert not failures, failures

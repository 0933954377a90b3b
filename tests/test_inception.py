"""Host logic of the native Inception-v3 (models/inception.py) over the emulator: module tree, BatchNorm folding, channel-slice
plan, re-packing, and the wiring into inception_utils / FIDComponent / calculate_inception_moments.  The kernels themselves
are checked on the GPU in test_inception_gpu.py."""
import argparse
import os
import types

import numpy as np
import pytest
import torch

import inception_cases as IC
from second_order_cases import errors, violations
from tartangan_amd import backend, inception_utils
from tartangan_amd import calculate_inception_moments as CIM
from tartangan_amd.models.inception import Inception3


@pytest.fixture
def emulated():
    prev = backend._set_backend_for_testing(IC.InceptionEmulator())
    yield
    backend._set_backend_for_testing(prev)


@pytest.fixture(scope='module')
def state():
    return IC.procedural_state(0)


@pytest.fixture(scope='module')
def small(state):
    """75 x 75 (the network's minimum), batch 2: input, float64 and fp32 references."""
    x = IC.procedural_input(2, 75, seed=3)
    ref64 = IC.reference(state, torch.float64)
    IC.check_reference_health(ref64, x)
    return x, IC.results(ref64, x.double()), IC.results(IC.reference(state, torch.float32), x)


def test_state_dict_matches_the_restatement_and_the_published_count(state):
    ref = IC.RefInception3()
    net = Inception3()
    want = {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    got = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    assert list(got) == list(want) and got == want
    assert sum(p.numel() for p in net.parameters()) == 27161264          # torchvision's published figure, aux head included
    assert [n for n, _ in net.named_children()] == [n for n, _ in ref.named_children()]
    net.load_state_dict(state)
    no_aux = {k: v for k, v in state.items() if not k.startswith('AuxLogits.')}
    assert len(no_aux) < len(state)
    net.load_state_dict(no_aux)                                         # the published file with the aux head stripped
    assert torch.equal(net.state_dict()['Mixed_7c.branch_pool.bn.running_var'], state['Mixed_7c.branch_pool.bn.running_var'])
    ref.load_state_dict(net.state_dict())                               # ... and back
    bare = Inception3(aux_logits=False)
    bare.load_state_dict(state)                                         # aux entries are dropped when there is no aux head
    assert not any(k.startswith('AuxLogits.') for k in bare.state_dict())


def test_plan_multiply_accumulates_match_the_published_figure():
    net = Inception3()
    assert abs(net.macs(299, 299) - 5.71e9) <= 0.01 * 5.71e9, net.macs(299, 299)
    plan = net.plan(299, 299)
    assert (plan.out.C, plan.out.H, plan.out.W) == (2048, 8, 8)
    convs = [op for op in plan.ops if op[0] == 'conv']
    assert sum(len(g) for g in plan.groups) == 94 and len(convs) < 94    # every conv once; shared-input 1x1 branches stacked
    kinds = {(op[8], op[9], op[10], op[11], op[12]) for op in convs}     # (KH, KW, stride, ph, pw)
    assert {(1, 1, 1, 0, 0), (3, 3, 2, 0, 0), (3, 3, 1, 0, 0), (3, 3, 1, 1, 1), (5, 5, 1, 2, 2), (1, 7, 1, 0, 3), (7, 1, 1, 3, 0),
            (1, 3, 1, 0, 1), (3, 1, 1, 1, 0)} == kinds
    with pytest.raises(ValueError, match='too small'):
        net.plan(74, 74)


def test_eval_only_and_forward_only(emulated, state):
    net = Inception3()
    assert not net.training and not net.train().training and not net.Mixed_5b.branch1x1.bn.training
    net.load_state_dict(state)
    x = IC.procedural_input(1, 75).requires_grad_(True)
    with pytest.raises(RuntimeError, match='forward-only'):
        net(x)
    with torch.no_grad():
        pool, logits = net(x)
    assert pool.shape == (1, 2048) and logits.shape == (1, 1000) and not pool.requires_grad


def test_native_forward_against_float64(emulated, state, small):
    x, r64, r32 = small
    net = Inception3()
    net.load_state_dict(state)
    got = IC.results(net, x)
    errs = errors(got, r64, r32)
    for k, e in errs.items():
        print(k, 'e_op %.2e e_32 %.2e max %.2e max_32 %.2e' % e[:4])
    assert not violations(errs), violations(errs)
    # buffers are cached per batch size and reused
    a = net.features(x)
    assert net.features(x).data_ptr() == a.data_ptr() and len(net._act_buffers) == 1
    net(IC.procedural_input(1, 75))
    assert len(net._act_buffers) == 2


def test_repacking_follows_the_parameters(emulated, state, small):
    x, r64, r32 = small
    net = Inception3()
    net.load_state_dict(IC.procedural_state(5))
    other = IC.results(net, x)
    net.load_state_dict(state)                                           # a second state dict: the next forward reflects it
    got = IC.results(net, x)
    assert not violations(errors(got, r64, r32))
    assert not torch.equal(other['pool'], got['pool'])
    net.Mixed_7c.branch1x1.bn.running_mean.add_(0.25)                    # a buffer written in place
    changed = dict(state)
    changed['Mixed_7c.branch1x1.bn.running_mean'] = state['Mixed_7c.branch1x1.bn.running_mean'] + 0.25
    ref = IC.reference(changed, torch.float64)
    assert not violations(errors(IC.results(net, x), IC.results(ref, x.double()), IC.results(IC.reference(changed, torch.float32), x)))
    assert not torch.equal(IC.results(net, x)['pool'], got['pool'])


def test_wrap_inception_runs_the_native_network(emulated, state):
    net = Inception3()
    net.load_state_dict(state)
    wrap = inception_utils.WrapInception(net)
    s = torch.rand(2, 3, 20, 20, generator=torch.Generator().manual_seed(2)) * 2 - 1
    ref = IC.reference(state, torch.float64)
    with torch.no_grad():
        pool, logits = wrap.forward_samples(s)
        pool2, _ = wrap.forward_samples(-s)
        want = ref(inception_utils.inception_preprocess(s, (299, 299), 2).double())
    assert pool.data_ptr() != pool2.data_ptr() and not torch.equal(pool, pool2)      # copies, not the cached buffers
    assert torch.allclose(pool.double(), want[0], rtol=1e-3, atol=1e-4)
    assert torch.allclose(logits.double(), want[1], rtol=1e-3, atol=1e-4)


def test_load_inception_net_from_a_weights_file(emulated, state, tmp_path, monkeypatch):
    path = os.path.join(tmp_path, 'inception_v3.pth')
    torch.save(state, path)
    monkeypatch.delenv('TG_INCEPTION_WEIGHTS', raising=False)
    wrap = inception_utils.load_inception_net(weights=path)
    assert isinstance(wrap, inception_utils.WrapInception) and isinstance(wrap.net, Inception3)
    assert torch.equal(wrap.net.fc.weight, state['fc.weight'])
    monkeypatch.setenv('TG_INCEPTION_WEIGHTS', path)
    via_env = inception_utils.load_inception_net()
    assert isinstance(via_env.net, Inception3) and torch.equal(via_env.net.Conv2d_1a_3x3.conv.weight, state['Conv2d_1a_3x3.conv.weight'])
    monkeypatch.delenv('TG_INCEPTION_WEIGHTS')
    with pytest.raises(RuntimeError, match='pass a loaded torchvision Inception3 as `net`'):     # neither: the old error
        inception_utils.load_inception_net()
    bad = os.path.join(tmp_path, 'bad.pth')
    torch.save({'x': torch.zeros(1)}, bad)
    with pytest.raises(RuntimeError, match='not an Inception-v3 state dict'):
        inception_utils.load_inception_net(weights=bad)


def _moments_file(tmp_path, seed=7):
    gen = torch.Generator().manual_seed(seed)
    data = torch.randn(64, 2048, generator=gen).double().numpy() * 0.1 + 0.3
    path = os.path.join(tmp_path, 'moments.npz')
    np.savez(path, mu=data.mean(0), sigma=np.cov(data, rowvar=False))
    return path


def test_fid_component_with_inception_weights(emulated, state, tmp_path, monkeypatch):
    from tartangan_amd.trainers.components import FIDComponent
    monkeypatch.delenv('TG_INCEPTION_WEIGHTS', raising=False)
    p = argparse.ArgumentParser()
    FIDComponent.add_args_to_parser(p)
    assert p.parse_args([]).inception_weights is None
    weights = os.path.join(tmp_path, 'w.pth')
    torch.save(state, weights)
    flags = p.parse_args(['--n-inception-imgs', '10', '--fid-freq', '1', '--inception-weights', weights,
                          '--inception-moments', _moments_file(tmp_path)])
    gen = torch.Generator().manual_seed(0)
    trainer = types.SimpleNamespace(args=flags, device='cpu', sample_g=lambda: torch.rand(2, 3, 16, 16, generator=gen) * 2 - 1)
    fid = FIDComponent(flags)
    fid.trainer = trainer
    fid.on_train_begin(0, {})
    logs = {}
    fid.on_batch_end(1, logs)
    assert set(logs) == {'fid', 'inception_score_mean', 'inception_score_std'}
    assert all(len(v) == 1 and np.isfinite(v[0]) for v in logs.values()) and logs['inception_score_mean'][0] >= 1.0 - 1e-5


def test_calculate_inception_moments_equals_numpy(emulated, state, tmp_path, capsys, monkeypatch):
    net = Inception3()
    net.load_state_dict(state)
    gen = torch.Generator().manual_seed(1)
    batches = [torch.randn(2, 3, 12, 12, generator=gen) for _ in range(5)]
    mu, sigma = CIM.calculate_inception_moments(iter(batches), net=net)
    assert 'Inception score of the data' in capsys.readouterr().out
    wrap = inception_utils.WrapInception(net)
    with torch.no_grad():
        pool = np.concatenate([wrap(b)[0].numpy() for b in batches], 0)
    assert mu.shape == (2048,) and sigma.shape == (2048, 2048)
    assert np.array_equal(mu, np.mean(pool, axis=0)) and np.array_equal(sigma, np.cov(pool, rowvar=False))

    # the command line: an image archive in, the .npz that --inception-moments reads out
    images = (torch.rand(10, 16, 16, 3, generator=gen) * 255).to(torch.uint8).numpy()
    source, dest, weights = (os.path.join(tmp_path, n) for n in ('images.npz', 'moments.npz', 'w.pth'))
    np.savez_compressed(source, images=images)
    torch.save(state, weights)
    monkeypatch.delenv('TG_INCEPTION_WEIGHTS', raising=False)
    torch.manual_seed(0)
    CIM.main([source, dest, '--batch-size', '2', '--inception-weights', weights, '--device', 'cpu', '--quiet-logs'])
    data = np.load(dest)
    assert data['mu'].shape == (2048,) and data['sigma'].shape == (2048, 2048) and np.isfinite(data['sigma']).all()
    get = inception_utils.prepare_inception_metrics(dest, 'cpu', no_fid=True, net=wrap)       # ... and it is read back
    sample_gen = torch.Generator().manual_seed(3)
    is_mean, is_std, fid_value = get(lambda: torch.rand(2, 3, 16, 16, generator=sample_gen) * 2 - 1, 4, num_splits=2)
    assert np.isfinite([is_mean, is_std, fid_value]).all()

"""The text kernels' host logic on the CPU: ``functional.conv1d`` / ``upsample_nearest2x_1d`` / ``avg_pool2_1d`` (first order by
gradcheck, an R1-style double backward against torch's own conv1d graph), ``functional.skipgram_step`` / ``embed_gather_t`` /
``embed_lookup``, ``models.text.SkipGram`` and the 1-D layer modules, run over float64 forms of the new entry points
(text_cases.TextEmulator).  Nothing here says anything about the HIP kernels (tests/test_conv1d_gpu.py,
test_embedding_skipgram_gpu.py)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import text_cases as TC
from tartangan_amd import backend, functional as TF
from tartangan_amd.models import layers as TL
from tartangan_amd.models.text import SkipGram


@pytest.fixture(autouse=True)
def emulated_backend():
    prev = backend._set_backend_for_testing(TC.TextEmulator())
    yield
    backend._set_backend_for_testing(prev)


def _rnd(*shape, seed=0, dtype=torch.float64):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed + sum(shape)), dtype=dtype)


# ------------------------------------------------------------------------------------------------------- first order
@pytest.mark.parametrize('ks', [1, 3])
def test_conv1d_gradcheck(ks):
    x, w, b, r = (_rnd(*s, seed=i).requires_grad_(True) for i, s in enumerate(((2, 3, 5), (4, 3, ks), (4,), (2, 4, 5))))
    assert torch.autograd.gradcheck(TF.conv1d, (x, w, b, r))
    assert torch.autograd.gradcheck(lambda x, w: TF.conv1d(x, w), (x, w))
    want = F.conv1d(x, w, b, padding=ks // 2) + r
    assert float((TF.conv1d(x, w, b, r) - want).detach().abs().max()) < 1e-12


def test_resamplers_gradcheck_and_values():
    x, r = _rnd(2, 3, 6).requires_grad_(True), _rnd(2, 3, 3, seed=1).requires_grad_(True)
    assert torch.autograd.gradcheck(TF.upsample_nearest2x_1d, (x,))
    assert torch.autograd.gradcheck(TF.avg_pool2_1d, (x, r))
    assert torch.autograd.gradgradcheck(TF.avg_pool2_1d, (x, r))
    assert torch.equal(TF.upsample_nearest2x_1d(x), F.interpolate(x, scale_factor=2))
    x = x.detach()
    assert float((TF.avg_pool2_1d(x) - F.avg_pool1d(x, 2)).abs().max()) < 1e-15
    # the discriminator block's shortcut: linear x0.5 without align_corners on an even length is the pair average
    assert float((TF.avg_pool2_1d(x) - F.interpolate(x, scale_factor=0.5, mode='linear', align_corners=False)).abs().max()) == 0.0
    with pytest.raises(RuntimeError):
        TF.avg_pool2_1d(_rnd(1, 1, 5))


# ------------------------------------------------------------------------------------------------------ second order
def _r1_net(ops, x, p):
    h = ops['elu'](ops['conv'](ops['up'](x), p['w1'], p['b1'], None))
    h = ops['pool'](ops['elu'](ops['conv'](h, p['w2'], p['b2'], None)), None)
    return ops['conv'](h, p['w3'], None, x)              # a k=1 layer with the block's shortcut in its epilogue


def _r1_grads(ops, x, p):
    """The R1 pattern of models/losses.py:17-30: grad of the output sum w.r.t. the input with create_graph, its squared norm added
    to the loss, one backward into the parameters."""
    x = x.detach().clone().requires_grad_(True)
    p = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    out = _r1_net(ops, x, p)
    g, = torch.autograd.grad(out.sum(), x, create_graph=True)
    loss = out.mean() + 0.5 * g.pow(2).sum(dim=(1, 2)).mean()
    grads = torch.autograd.grad(loss, list(p.values()))
    return [loss.detach()] + list(grads)


TORCH_OPS = dict(conv=lambda x, w, b, r: F.conv1d(x, w, b, padding=w.shape[2] // 2) + (0 if r is None else r),
                 up=lambda x: F.interpolate(x, scale_factor=2), pool=lambda x, r: F.avg_pool1d(x, 2) + (0 if r is None else r), elu=F.elu)
HIP_OPS = dict(conv=TF.conv1d, up=TF.upsample_nearest2x_1d, pool=TF.avg_pool2_1d, elu=TF.elu)


def check_r1_double_backward(device, dtype):
    """conv1d / resamplers differentiated twice, against torch's own conv1d graph in float64.  In float64 (the emulator) the two
    agree to roundoff; in float32 (the device) by the house rule, e32 being torch's own float32 graph on the CPU."""
    B, C, L = 3, 5, 6
    x = _rnd(B, C, L)
    p = dict(w1=_rnd(7, C, 3, seed=1) * 0.4, b1=_rnd(7, seed=2), w2=_rnd(6, 7, 3, seed=3) * 0.4, b2=_rnd(6, seed=4), w3=_rnd(C, 6, 1, seed=5) * 0.4)
    want = _r1_grads(TORCH_OPS, x, p)
    got = _r1_grads(HIP_OPS, x.to(device, dtype), {k: v.to(device, dtype) for k, v in p.items()})
    if dtype == torch.float64:
        limits = [1e-11] * len(want)
    else:
        r32 = _r1_grads(TORCH_OPS, x.float(), {k: v.float() for k, v in p.items()})
        limits = [TC.limit(TC.rel(r, w)) for r, w in zip(r32, want)]
    names = ['loss'] + list(p)
    failures = []
    for n, g, w, lim in zip(names, got, want, limits):
        err = TC.rel(g.cpu(), w)
        print(f'R1-1D {n}: err {err:.2e} limit {lim:.2e}')
        if err > lim:
            failures.append((n, err, lim))
    assert not failures, failures


def test_r1_style_double_backward_against_torchs_conv1d_graph():
    check_r1_double_backward('cpu', torch.float64)


# ---------------------------------------------------------------------------------------------------------- skip-gram
@pytest.mark.parametrize('variant,shape', [('plain', (4, 6, 8, 23)), ('plain', (5, 4, 100, 7)), ('same_word', (16, 4, 8, 23)),
                                           ('padding', (6, 4, 8, 23))])
def test_skipgram_train_step_is_the_references_sparse_sgd_step(variant, shape):
    """Against the reference's own procedure in float64: nn.Embedding(sparse=True, padding_idx) tables, SkipGram.loss's ops, backward
    (sparse gradients, coalesced by the optimiser) and torch.optim.SGD -- with duplicate rows and padding rows."""
    B, C2, E, vocab = shape
    lr = 0.7
    c = TC.skipgram_case(B, C2, E, vocab, lr, variant)
    pad = c['padding_idx'] if c['padding_idx'] >= 0 else None
    ref_u, ref_v = (nn.Embedding(vocab, E, sparse=True, padding_idx=pad).double() for _ in range(2))
    with torch.no_grad():
        ref_u.weight.copy_(c['U'])
        ref_v.weight.copy_(c['V'])
    opt = torch.optim.SGD(list(ref_u.parameters()) + list(ref_v.parameters()), lr=lr)
    emb_u = ref_u(c['words'])
    scores = torch.bmm(ref_v(c['contexts']), emb_u.unsqueeze(-1)).squeeze(-1)
    negative_scores = torch.bmm(ref_v(c['negatives']), emb_u.unsqueeze(-1)).squeeze(-1)
    ref_loss = -(F.logsigmoid(scores).sum(1) + F.logsigmoid(-negative_scores).sum(1)).mean()
    ref_loss.backward()
    assert ref_u.weight.grad.is_sparse
    opt.step()
    ref_loss = ref_loss.detach()

    m = SkipGram(vocab, E, sparse=True, padding_idx=pad).double()
    assert list(m.state_dict()) == ['embedding_u.weight', 'embedding_v.weight']
    m.load_state_dict({'embedding_u.weight': c['U'].double(), 'embedding_v.weight': c['V'].double()})
    loss = m.train_step(c['words'], c['contexts'], c['negatives'], lr)
    assert abs(float(loss) - float(ref_loss)) <= 1e-12 * abs(float(ref_loss))
    assert float((m.embedding_u.weight - ref_u.weight).detach().abs().max()) <= 1e-12
    assert float((m.embedding_v.weight - ref_v.weight).detach().abs().max()) <= 1e-12
    tu, tv = TC.untouched_rows(c, vocab)
    assert torch.equal(m.embedding_u.weight.detach()[tu], c['U'].double()[tu]) and torch.equal(m.embedding_v.weight.detach()[tv], c['V'].double()[tv])
    assert m.embedding_u.weight.grad is None and m.embedding_v.weight.grad is None          # outside autograd


def test_skipgram_negatives_follow_the_references_stream():
    m = SkipGram(50, 4)
    contexts = torch.zeros(6, 4, dtype=torch.int64)
    torch.manual_seed(5)
    want = torch.randint_like(contexts, 0, 50)
    after = torch.get_rng_state()
    torch.manual_seed(5)
    assert torch.equal(m.draw_negatives(contexts), want) and torch.equal(torch.get_rng_state(), after)


def test_indexes_outside_the_vocabulary_raise_on_the_host():
    m = SkipGram(7, 4).double()
    ok = torch.zeros(2, 2, dtype=torch.int64)
    with pytest.raises(IndexError):
        m.train_step(torch.tensor([0, 7]), ok, ok, 0.1)
    with pytest.raises(IndexError):
        m.gather_t(torch.tensor([[-1, 2]]))


def test_forward_gather_and_lookup_follow_the_reference():
    c = TC.lookup_case(3, 7, 8, 23)
    assert TC.lookup_margin(c['U'], c['z']) >= TC.LOOKUP_MARGIN
    m = SkipGram(23, 8, padding_idx=0)
    m.embedding_u.weight.data.copy_(c['U'])
    # the reference's lookup, verbatim ops
    w = m.embedding_u.weight.detach().double()
    w_norm = w.pow(2).sum(1).sqrt()[..., None]
    want = [torch.argmax((torch.mm(w, z) / w_norm)[1:], dim=0) for z in c['z'].double()]
    got = m.lookup(c['z'])
    assert len(got) == 3 and all(torch.equal(g, t) for g, t in zip(got, want))
    idx = torch.randint(0, 23, (4, 9), generator=torch.Generator().manual_seed(2))
    assert torch.equal(m.gather_t(idx), m.embedding_u(idx).permute(0, 2, 1).detach())
    assert torch.equal(m(idx), m.embedding_u(idx).detach()) and not m(idx).requires_grad


# -------------------------------------------------------------------------------------------------------------- layers
def test_layer_modules_match_their_torch_parents():
    torch.manual_seed(0)
    x = torch.randn(4, 6, 8)
    for ks in (1, 3):
        conv = TL.Conv1d(6, 5, ks, padding=ks // 2)
        assert list(conv.state_dict()) == list(nn.Conv1d(6, 5, ks).state_dict())
        assert float((conv(x) - nn.Conv1d.forward(conv, x)).abs().max()) < 1e-5
    with pytest.raises(ValueError):
        TL.Conv1d(6, 5, 5, padding=2)
    with pytest.raises(ValueError):
        TL.Conv1d(6, 5, 3, padding=0)
    assert float((TL.AvgPool1d(2)(x) - F.avg_pool1d(x, 2)).abs().max()) < 1e-6
    bn, ref = TL.BatchNorm1d(6), nn.BatchNorm1d(6)
    assert list(bn.state_dict()) == list(ref.state_dict())
    assert float((bn(x) - ref(x)).abs().max()) < 1e-5 and float((bn.running_var - ref.running_var).abs().max()) < 1e-6
    assert float((bn.forward_act(x, 0.2) - F.leaky_relu(ref(x), 0.2)).abs().max()) < 1e-5
    bn.eval(), ref.eval()
    assert float((bn(x) - ref(x)).abs().max()) < 1e-5
    assert torch.equal(TL.interpolate(x, scale_factor=2), F.interpolate(x, scale_factor=2))
    half = TL.Interpolate(scale_factor=0.5, mode='linear', align_corners=False)
    assert float((half(x) - F.interpolate(x, scale_factor=0.5, mode='linear', align_corners=False)).abs().max()) < 1e-6
    with pytest.raises(NotImplementedError):
        half(torch.randn(1, 2, 7))
    with pytest.raises(NotImplementedError):
        TL.interpolate(x, scale_factor=0.5, mode='linear', align_corners=True)


# --------------------------------------------------------------------------------------------------------- the 1-D models
def text_models_pair(config_name, E, norm, activation, dtype=torch.float64, seed=3):
    """(g, d) on the HIP layer classes and (g, d) on stock torch.nn layers with the same weights (one procedural state)."""
    from oracle.procedural import procedural_state
    from tartangan_amd.models.pluggan import GAN_CONFIGS
    from tartangan_amd.models.text import build_text_models
    cfg = GAN_CONFIGS[config_name]._replace(data_dims=E)
    mine, stock = build_text_models(cfg, norm, activation), build_text_models(cfg, norm, activation, layers=nn)
    for k, (a, b) in enumerate(zip(mine, stock)):
        assert list(a.state_dict()) == list(b.state_dict())
        state = procedural_state(b.state_dict(), seed + k)
        a.load_state_dict(state)
        b.load_state_dict(state)
        a.to(dtype), b.to(dtype)
    return cfg, mine, stock


def check_text_models(device, dtype, bound):
    """G's sample, D's logits and an R1-penalised D step's parameter gradients on the HIP layers against stock torch.nn layers in
    float64 on the CPU (Conv1d, BatchNorm1d, AvgPool1d, F.interpolate 'linear'), relative to the largest reference value."""
    for config_name, E, norm, activation in (('16', 8, 'bn', 'relu'), ('32', 16, 'id', 'elu')):
        cfg, (g, d), (g_ref, d_ref) = text_models_pair(config_name, E, norm, activation)
        g, d = g.to(device, dtype), d.to(device, dtype)
        z, real = _rnd(4, cfg.latent_dims, seed=9), _rnd(4, E, g.max_size, seed=10)

        def d_step(net, x):
            x = x.clone().requires_grad_(True)
            p = net(x)
            gx, = torch.autograd.grad(p.sum(), x, create_graph=True)
            loss = F.softplus(-p).mean() + 5.0 * gx.pow(2).flatten(1).sum(1).mean()
            return [p.detach()] + list(torch.autograd.grad(loss, list(net.parameters())))
        # the stock-layer side always runs on the CPU in float64 (its Linear and sum pool over the emulator)
        prev = backend._set_backend_for_testing(TC.TextEmulator())
        try:
            fake_ref, grads_ref = g_ref(z).detach(), d_step(d_ref, real)
        finally:
            backend._set_backend_for_testing(prev)
        fake = g(z.to(device, dtype))
        assert tuple(fake.shape) == (4, E, g.max_size)
        assert TC.rel(fake.detach().cpu(), fake_ref) <= bound
        grads = [d_step(d, real.to(device, dtype)), grads_ref]
        # (a bias in front of a BatchNorm has a gradient of exactly zero in exact arithmetic: what both sides hold there is roundoff,
        # so a tensor is measured against the larger of its own largest value and the largest parameter gradient of the network)
        largest = max(float(b.abs().max()) for b in grads[1][1:])
        for name, a, b in zip(['logits'] + [n for n, _ in d.named_parameters()], *grads):
            err = float((a.cpu().double() - b).abs().max()) / max(float(b.abs().max()), largest if name != 'logits' else 0.)
            assert err <= bound, (config_name, name, err)


def test_text_models_match_stock_torch_layers_including_the_r1_step():
    check_text_models('cpu', torch.float64, 1e-9)


def test_text_models_have_the_reference_layout_and_refuse_attention():
    from tartangan_amd.models.pluggan import GAN_CONFIGS
    from tartangan_amd.models.text import build_text_models
    g, d = build_text_models(GAN_CONFIGS['16']._replace(data_dims=8))
    keys = list(g.state_dict())
    assert keys[:2] == ['blocks.0.base.0.weight', 'blocks.0.base.0.bias'] and g.blocks[0].base[0].weight.shape == (4 * 64, 100)
    assert g.blocks[1].convs[0].weight.shape == (64, 64, 3) and g.blocks[-1].convs[2].weight.shape == (8, 32, 1)
    assert isinstance(g.blocks[-1].convs[3], nn.Identity) and isinstance(d.blocks[1].convs[1], TL.BatchNorm1d)      # D gets G's norm
    assert d.blocks[0].convs[0].weight.shape == (32, 8, 1) and g.max_size == 16
    with pytest.raises(NotImplementedError):
        build_text_models(GAN_CONFIGS['512thin']._replace(data_dims=8))


# -------------------------------------------------------------------------------------------------------------- dataset
def test_text_dataset_tokens_vocabulary_order_padding_and_cut():
    from tartangan_amd.text_dataset import TextDataset, basic_english
    assert basic_english("Hello, World! It's (not) \"quoted\"; a:b <br /> end.") == \
        ['hello', ',', 'world', '!', 'it', "'", 's', '(', 'not', ')', 'quoted', 'a', 'b', 'end', '.']
    docs = {'summary': ['the cat sat. the dog sat!', 'a cat, a dog, a bird', 'zebra']}
    ds = TextDataset(docs, doc_len=6)
    # specials first, then by falling count, equal counts alphabetically: a 3; , 2, cat 2, dog 2, sat 2, the 2; the rest 1
    assert ds.vocab.itos == ['<unk>', '<pad>', 'a', ',', 'cat', 'dog', 'sat', 'the', '!', '.', 'bird', 'zebra']
    assert len(ds.vocab) == 12 and len(ds) == 3
    assert ds.vocab.stoi['<PAD>'] == 0 and ds.vocab.stoi['never seen'] == 0 and 'never seen' not in ds.vocab.stoi
    assert ds[0].tolist() == [7, 4, 6, 9, 7, 5]                  # cut to doc_len
    assert ds[2].tolist() == [11, 0, 0, 0, 0, 0] and ds[2].dtype == np.int64      # zero padded
    assert ds[1].tolist() == [2, 4, 3, 2, 5, 3]
    import pandas as pd
    assert TextDataset(pd.DataFrame(docs), doc_len=6).vocab.itos == ds.vocab.itos


# -------------------------------------------------------------------------------------------------------------- trainer
def run_fixture_steps(fx, device):
    """This package's trainer from the fixture's state over the fixture's batches -> (trainer, [step entries])."""
    tr = TC.text_trainer(fx, device)
    TC.load_procedural(tr, fx)
    TC.seed_step_streams(fx)
    entries = [TC.step_entry(tr, tr.train_batch(TC.documents(fx, k))) for k in range(fx['n_steps'])]
    return tr, entries


def check_trainer_against_fixture(case, device, bound=1e-4):
    """Every loss and norm of every step within ``bound`` of what the reference's own trainer recorded, both host streams where the
    reference left them, the reference's state_dict keys."""
    fx = TC.load_text_fixture(case)
    tr, entries = run_fixture_steps(fx, device)
    failures = []
    for k, (got, want) in enumerate(zip(entries, fx['steps'])):
        for key, ref in want.items():
            if key not in got:
                assert key in ('u_grad_l2', 'v_grad_l2')        # the fused skip-gram step keeps no table gradient
                continue
            dev = abs(got[key] - ref) / abs(ref) if ref else abs(got[key])
            print(f'TEXT {case} [{device}] step {k + 1} {key}: {got[key]:.7g} reference {ref:.7g} dev {dev:.2e}')
            if dev > bound:
                failures.append((k + 1, key, got[key], ref, dev))
    assert not failures, failures
    assert dict(torch=float(torch.rand(1)), numpy=float(np.random.rand())) == fx['rng_after']
    assert list(tr.g.state_dict()) == fx['state_keys']['g'] == list(tr.target_g.state_dict())
    assert list(tr.d.state_dict()) == fx['state_keys']['d'] and list(tr.embedding.state_dict()) == fx['state_keys']['embedding']


@pytest.mark.parametrize('case', TC.TEXT_CASES)
def test_trainer_against_the_reference_fixtures(case):
    check_trainer_against_fixture(case, 'cpu')


def test_pretraining_counter_and_the_embedding_only_step():
    fx = TC.load_text_fixture('text_c16_e8_b4')
    tr = TC.text_trainer(fx, 'cpu')
    TC.load_procedural(tr, fx)
    TC.seed_step_streams(fx)
    assert tr.pretraining_embedding == 2
    snap = lambda m: [p.detach().clone() for p in m.parameters()]
    g0, d0, t0, e0 = snap(tr.g), snap(tr.d), snap(tr.target_g), snap(tr.embedding)
    bn0 = [b.clone() for b in tr.d.buffers()]
    logs = tr.train_batch(TC.documents(fx, 0))
    assert tr.pretraining_embedding == 1 and logs['g_loss'] == logs['d_loss'] == logs['gp'] == 0. and logs['embedding_loss'] > 0
    same = lambda a, b: all(torch.equal(x, y) for x, y in zip(a, b))
    assert same(g0, snap(tr.g)) and same(d0, snap(tr.d)) and same(bn0, list(tr.d.buffers()))          # G and D bit-unchanged
    assert not same(t0, snap(tr.target_g)) and not same(e0, snap(tr.embedding))                       # the target and the tables move
    logs = tr.train_batch(TC.documents(fx, 1))
    assert tr.pretraining_embedding == 0 and logs['g_loss'] > 0 and logs['d_loss'] > logs['gp'] > 0   # d_loss includes the penalty
    assert not same(g0, snap(tr.g)) and not same(d0, snap(tr.d))
    tr.train_batch(TC.documents(fx, 2))
    assert tr.pretraining_embedding == 0 and tr.steps == 3


def test_target_generator_is_not_a_copy_at_start_and_d_keeps_gs_norm():
    fx = TC.load_text_fixture('text_c16_e8_b4')
    tr = TC.text_trainer(fx, 'cpu')
    assert not all(torch.equal(a, b) for a, b in zip(tr.g.parameters(), tr.target_g.parameters()))
    assert any(isinstance(m, TL.BatchNorm1d) for m in tr.d.modules())
    tr_id = TC.text_trainer(fx, 'cpu', norm='id')
    assert not any(isinstance(m, TL.BatchNorm1d) for m in list(tr_id.d.modules()) + list(tr_id.g.modules()))


def test_refusals_graphs_data_parallel_and_attention():
    fx = TC.load_text_fixture('text_c16_e8_b4')
    tr = TC.text_trainer(fx, 'cpu')
    with pytest.raises(NotImplementedError, match='graph'):
        tr.enable_graphs()
    tr.data_parallel = object()
    with pytest.raises(NotImplementedError, match='world'):
        tr.train_batch(TC.documents(fx, 0))
    from tartangan_amd.models.pluggan import GAN_CONFIGS
    from tartangan_amd.trainers.text_cnn import TextCNNTrainer
    bad = TextCNNTrainer(TextCNNTrainer.default_args(config=GAN_CONFIGS['32']._replace(attention=(1,)), device='cpu', embedding_dims=8))
    with pytest.raises(NotImplementedError, match='attention'):
        bad.build_models()
    from tartangan_amd.trainers.trainer import RngFeed
    feed = RngFeed('cpu')
    with pytest.raises(NotImplementedError):
        feed.draw('offsets', 4, 7)                   # (mode 'record': the integer kinds are inline-only)


def test_sampler_writes_its_file(tmp_path):
    from tartangan_amd.text_dataset import TextDataset
    from tartangan_amd.trainers.components.text_sampler import TextSamplerComponent
    from tartangan_amd.trainers.text_cnn import TextCNNTrainer
    docs = {'summary': ['the cat sat on the mat. the dog sat too!', 'a bird, a cat and a dog walk in', 'zebra crossing ahead']}
    tr = TextCNNTrainer(TextCNNTrainer.default_args(config='16', batch_size=2, device='cpu', embedding_dims=8, pretrain_embedding=0,
                                                    output=str(tmp_path), run_id='r', gen_freq=2))
    torch.manual_seed(0)
    tr.build_models()
    tr.dataset = TextDataset(docs, doc_len=tr.g.max_size)
    tr.build_embedding(len(tr.dataset.vocab), tr.dataset.vocab.stoi['<PAD>'])
    sampler = TextSamplerComponent()
    tr.attach(sampler)
    torch.manual_seed(3)
    want_z = torch.randn(32, tr.gan_config.latent_dims)
    torch.manual_seed(3)
    sampler.on_train_begin(0, {})
    assert torch.equal(sampler.progress_samples, want_z)
    sampler.on_batch_end(1, {})
    assert not (tmp_path / 'r' / 'samples' / 'sample_1.txt').exists()
    sampler.on_batch_end(2, {})
    text = (tmp_path / 'r' / 'samples' / 'sample_2.txt').read_text()
    blocks = text.split('-' * 40 + '\n')
    assert len(blocks) == 17 and blocks[-1] == ''
    words = blocks[0].split()
    assert len(words) == tr.g.max_size and set(words) <= set(tr.dataset.vocab.itos) and all(len(l) <= 70 for l in text.splitlines())
    # decoded exactly as the reference does: itos[index returned by lookup], the row-0 quirk included
    with torch.no_grad():
        idx = tr.embedding.lookup(tr.g(sampler.progress_samples)[:1])[0]
    assert words == [tr.dataset.vocab.itos[i] for i in idx.tolist()]
    logs = tr.train_batch(np.stack([tr.dataset[0], tr.dataset[1]]))
    assert set(logs) == {'g_loss', 'd_loss', 'gp', 'embedding_loss'}


def test_cli_parser_accepts_the_references_arguments():
    import argparse
    from tartangan_amd.trainers.text_cnn import TextCNNTrainer
    p = argparse.ArgumentParser()
    TextCNNTrainer.add_args_to_parser(p)
    a = p.parse_args([])
    assert (a.embedding_dims, a.context, a.pretrain_embedding, a.config, a.batch_size, a.norm, a.activation, a.g_base) == \
        (64, 3, 10000, '64', 128, 'bn', 'relu', 'mlp')
    a = p.parse_args('--embedding-dims 32 --context 2 --pretrain-embedding 5 --norm id --activation selu --g-base mlp --config 32 '
                     '--lr-d 1e-3 --lr-g 2e-4 --lr-target-g 1e-2 --grad-penalty 0 --batch-size 16 --model-scale 0.5'.split())
    assert (a.embedding_dims, a.context, a.pretrain_embedding, a.norm, a.activation, a.lr_d, a.grad_penalty) == (32, 2, 5, 'id', 'selu', 1e-3, 0.)
    tr = TextCNNTrainer(TextCNNTrainer.default_args(config='16', device='cpu', embedding_dims=8, activation='selu', g_base='mlp'))
    tr.build_models()                                  # the selu initialisation runs
    with pytest.raises(KeyError):
        TextCNNTrainer(TextCNNTrainer.default_args(config='16', device='cpu', embedding_dims=8, g_base='tiledz')).build_models()

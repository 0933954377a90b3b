"""Synchronised BatchNorm on the HIP library against float64.

(a) The kernels: the cases of tests/sync_bn_cases.py -- W ranks in lockstep in one process through the C ABI
    (tg_bn_sync_{stats,bwd,dbwd}_{local,finish}), stock torch on the global batch as the reference -- with the rule of
    tests/second_order_cases.py, "no worse than plain fp32".  Edge shapes, unaligned tensors, a large common offset, exact edges,
    rank counts 1 / 2 / 4 / 8, and the BatchNorm layers of the 128:3 generator and discriminator at per-rank batch 32.
(b) The sharded D phase: W gloo ranks on the one GPU run ``_d_phase`` under ``DataParallel(sync_bn=True)`` on their shards, and
    the averaged losses, every averaged D parameter gradient and D's BatchNorm buffers are compared with the float64 oracle at the
    GLOBAL batch, next to the same oracle in fp32: the SyncBN twin of test_d_phase_r1_gradients_match_float64_oracle."""
import os
import queue
import socket
import sys
import traceback

import pytest
import torch

import second_order_cases as SO
import sync_bn_cases as SB

pytestmark = pytest.mark.gpu

_REFS = {}


def _refs(spec):
    if spec.name not in _REFS:
        _REFS[spec.name] = SB.references(spec)
    return _REFS[spec.name]


@pytest.fixture(scope='module')
def K():
    from tartangan_amd import backend
    return backend.get()


# --------------------------------------------------------------------------- (a) the kernels
@pytest.mark.parametrize('spec', SB.edge_shape_specs() + SB.offset_specs() + SB.unaligned_specs() + SB.rank_constant_specs(), ids=repr)
def test_sync_passes_match_float64_torch_on_the_global_batch(K, spec):
    errs, bad = SB.run_case(K, 'cuda', spec, _refs(spec))
    torch.cuda.synchronize()
    SB.report(spec, errs)
    assert not bad, bad


def test_all_six_entry_points_are_reached_through_the_c_abi(K):
    assert K.name == 'hip'
    spec = SB.edge_shape_specs()[0]
    with SO.Recorder(K, SB.SYNC_ENTRY_POINTS + ('bn_act_fwd',)) as rec:
        errs, bad = SB.run_case(K, 'cuda', spec, _refs(spec))
    assert not bad, bad
    assert set(SB.SYNC_ENTRY_POINTS) <= set(rec.seen), sorted(rec.seen)
    assert all((spec.B, spec.C, spec.HW) == shape[:3] for n in ('bn_sync_stats_local', 'bn_sync_bwd_local', 'bn_sync_dbwd_local')
               for shape in rec.seen[n])


@pytest.mark.parametrize('shape', sorted(SB.invariance_specs()), ids=str)
def test_rank_count_invariance(K, shape):
    """One global batch over 1, 2, 4 and 8 ranks: every split within the rule, and W = 1 next to the local-statistics kernels."""
    group = SB.invariance_specs()[shape]
    t, r64, r32 = SB.references(group[0])
    failures = []
    for spec in group:
        errs, bad = SB.check(spec, SB.run_sync(K, 'cuda', spec, t), r64, r32)
        SB.report(spec, errs)
        failures += bad
    errs, bad = SB.check(group[0], SB.run_local(K, 'cuda', group[0], t), r64, r32)
    SB.report(group[0], errs, tag='SYNCBN local-kernels')
    assert not failures + bad, failures + bad


@pytest.mark.parametrize('spec', [SB.edge_shape_specs()[0], SB.edge_shape_specs()[9]], ids=repr)
def test_nullable_buffers_and_rejected_forms(K, spec):
    t, r64, r32 = _refs(spec)
    bad = SB.check_nullable_and_rejected_forms(K, 'cuda', spec, t, r64, r32)
    assert not bad, bad


@pytest.mark.parametrize('spec', [s for s in SB.edge_shape_specs() if s.replicate == 4][:4], ids=repr)
def test_replicate_moves_running_var_and_nothing_else(K, spec):
    SB.check_replicate_only_moves_running_var(K, 'cuda', spec, _refs(spec)[0])


@pytest.mark.parametrize('spec', SB.zero_specs(), ids=repr)
def test_lrelu_mask_at_exactly_zero_is_torchs(K, spec):
    SB.report(spec, SB.check_zero_edge(K, 'cuda', spec, _refs(spec)))


@pytest.mark.parametrize('spec', SB.constant_specs(), ids=repr)
def test_channel_constant_over_all_ranks(K, spec):
    SB.report(spec, SB.check_constant_edge(K, 'cuda', spec, _refs(spec)))


def test_network_layers_at_two_and_eight_ranks(K):
    """Every BatchNorm of the 128:3 generator and discriminator, recorded from one local-statistics step at batch 32, as 2 ranks
    of 32; as 8 ranks of 32 (the hardware configuration) where the global tensor stays below 2^25 elements."""
    two, eight = SB.layer_specs(SB.record_bn_layers(K, 'cuda'))
    assert len(two) >= 10 and any(s.replicate == 4 for s in two)
    failures, worst = [], {}
    for spec in two + eight:
        refs = SB.references(spec)
        errs, bad = SB.run_case(K, 'cuda', spec, refs)
        del refs
        SB.report(spec, errs)
        for p, r in SB.worst_ratios(errs).items():
            worst[(spec.W, p)] = max(worst.get((spec.W, p), 0.0), r)
        failures += bad
    print('SYNCBN layers worst ' + ' '.join(f'W{w}.{p}={r:.2f}' for (w, p), r in sorted(worst.items())))
    assert not failures, failures


# --------------------------------------------------------------------------- (b) the sharded D phase against the float64 oracle
SHARDED_CASES = [('c32a2_iqn_b8', (2,)), ('c64a1_cnn_b8', (2,)), ('c64a1_iqn_b8', (2,)), ('c64a1_iqn_b64', (2, 4)), ('c32_cnn_b8_selu', (2,))]
SEEDS = range(5)
BUFFER = 'buffer:'


def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _rank_d_phase(fx, seed, rank, world):
    """This rank's D phase on its shard (see hip_d_phase of test_second_order_gpu), gradients averaged over the ranks."""
    import torch.distributed as dist
    import test_second_order_gpu as T
    from conftest import trainer_from_fixture
    from oracle import sagan_cpu as O
    from tartangan_amd.parallel import DataParallel
    B = fx['batch']
    b = B // world
    ref = T._oracle(fx)
    tr = trainer_from_fixture(dict(fx, batch=b), 'cuda')
    tr.d.load_state_dict({k: v.clone() for k, v in ref.d.items()})
    dp = DataParallel(tr, sync_bn=True)
    real, fake, taus = T._d_phase_inputs(fx, seed)
    fake = dp.shard(fake).cuda()
    tr._generator_forward_for_both_phases = lambda bs: None
    tr.sample_g = lambda n=None, **kw: fake
    if taus is not None:
        # tau rows are quantile-major: this rank's images of every quantile
        feed = [t.view(O.NUM_QUANTILES, B, 1)[:, rank * b:(rank + 1) * b].reshape(-1, 1).cuda() for t in taus]
        heads = [m for m in tr.d.modules() if hasattr(m, 'tau_source')]
        assert len(heads) == 1
        heads[0].tau_source = lambda rows, nq: feed.pop(0)
    tr._training_mode()
    d_loss, gp = tr._d_phase(dp.shard(real).cuda())
    if taus is not None:
        assert not feed, 'the D phase did not draw both tau sets'
    dp.all_reduce_mean(tr.optimizer_d.grads)
    torch.cuda.synchronize()
    losses = torch.stack([d_loss, gp]).to('cpu', torch.float64)
    dist.all_reduce(losses)
    losses /= world
    flat = tr.optimizer_d.grads.cpu()
    bufs = {k: v.detach().cpu() for k, v in tr.d.state_dict().items() if 'running_' in k or 'num_batches_tracked' in k}
    packed = torch.cat([flat.double()] + [v.double().reshape(-1) for _, v in sorted(bufs.items())])
    gathered = [torch.zeros_like(packed) for _ in range(world)]
    dist.all_gather(gathered, packed)
    out = {'d_loss': losses[0], 'gp': losses[1]}
    out.update({k: p.grad for k, p in tr.d.named_parameters() if p.grad is not None})
    out = {k: v.detach().to('cpu', torch.float64) for k, v in out.items()}
    out.update({BUFFER + k: v for k, v in bufs.items()})
    out['replicas_equal'] = all(torch.equal(gathered[0], g) for g in gathered)
    return out


def _worker(rank, world, port, case, seeds, path, out):
    try:
        os.environ['MASTER_ADDR'] = '127.0.0.1'
        os.environ['MASTER_PORT'] = str(port)
        import torch.distributed as dist
        from conftest import load_golden
        torch.cuda.set_device(0)
        dist.init_process_group('gloo', rank=rank, world_size=world)
        fx = load_golden(case)
        res = [_rank_d_phase(fx, seed, rank, world) for seed in seeds]
        if rank == 0:
            torch.save(res, path)
        dist.barrier()
        dist.destroy_process_group()
        if rank == 0:
            out.put(('ok', rank, ''))
    except BaseException:
        out.put(('failed', rank, traceback.format_exc()))
        sys.exit(1)


def _sharded(case, world, seeds, path):
    """The per-seed results of rank 0.  One ``Queue.get``; whatever goes wrong, the workers are terminated, nothing is retried
    and nothing more is started for this case."""
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    out = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, case, list(seeds), str(path), out)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        status, rank, text = out.get(timeout=900)
    except queue.Empty:
        status, rank, text = 'timeout', -1, ''
    if status == 'ok':
        for p in procs:
            p.join(120)
    codes = [p.exitcode for p in procs]
    for p in procs:
        if p.is_alive():
            p.terminate()
    for p in procs:
        p.join(30)
    assert status == 'ok' and codes == [0] * world, f'{case} W={world}: {status} (rank {rank}), exit codes {codes}\n{text[-3000:]}'
    return torch.load(path)


def _oracles(fx, seed):
    import test_second_order_gpu as T
    return T.oracle_d_phase(fx, seed, torch.float64, buffers=BUFFER), T.oracle_d_phase(fx, seed, torch.float32, buffers=BUFFER)


@pytest.mark.parametrize('case,worlds', SHARDED_CASES, ids=[c for c, _ in SHARDED_CASES])
def test_sharded_d_phase_matches_float64_oracle_at_the_global_batch(case, worlds, tmp_path):
    """d_loss, gp, every D parameter gradient and D's running statistics after one D phase sharded over W ranks with SyncBN,
    against the float64 oracle at the global batch: median over the 5 image seeds of e_hip <= 4 max(median e_32, EPS) for every
    quantity.  num_batches_tracked: exactly the oracle's (the real pass, then the fake pass: += 2) on every rank.
    Measured worst ratios (two runs on an MI355X): c32a2_iqn_b8 1.16, c64a1_cnn_b8 2.38 / 2.57, c64a1_iqn_b8 3.98 / 3.99
    (blocks.2.project_input.0.bias, also the worst quantity of that fixture's single-GPU D phase), c64a1_iqn_b64 1.77 (W = 2) and
    2.62 (W = 4), c32_cnn_b8_selu 1.31; buffers at most 1.04."""
    from conftest import load_golden
    fx = load_golden(case)
    refs = [_oracles(fx, s) for s in SEEDS]                  # once, for every rank count
    failures = []
    for world in worlds:
        assert fx['batch'] % world == 0
        got = _sharded(case, world, SEEDS, tmp_path / f'{case}_w{world}.pt')
        per = {}
        for (r64, r32), hip in zip(refs, got):
            assert hip.pop('replicas_equal'), 'ranks disagree on the averaged gradients or on the BatchNorm buffers'
            assert set(hip) == set(r64), sorted(set(hip) ^ set(r64))
            for k, T64 in r64.items():
                if k.endswith('num_batches_tracked'):
                    assert int(hip[k]) == int(T64) == 2 and hip[k].dtype == torch.int64, (k, hip[k], T64)
                    continue
                n = float(T64.norm()) or 1.0
                per.setdefault(k, []).append((float((hip[k].double() - T64).norm()) / n, float((r32[k] - T64).norm()) / n))
        stats = {k: (sorted(e for e, _ in v)[len(v) // 2], sorted(e for _, e in v)[len(v) // 2]) for k, v in per.items()}
        ratio = lambda k: stats[k][0] / max(stats[k][1], SO.EPS)
        worst = max(stats, key=ratio)
        bufs = [k for k in stats if k.startswith(BUFFER)]
        print(f'SYNC_DPHASE W={world} {case} worst={worst} ratio={ratio(worst):.2f} gp={stats["gp"][0]:.2e}/{stats["gp"][1]:.2e} '
              f'd_loss={stats["d_loss"][0]:.2e}/{stats["d_loss"][1]:.2e}'
              + (f' worst_buffer={max(bufs, key=ratio)} ratio={ratio(max(bufs, key=ratio)):.2f}' if bufs else ''))
        failures += [f'W={world} {case} {k}: median e_hip {a:.2e} e_32 {b:.2e}' for k, (a, b) in stats.items()
                     if a > SO.RATIO_L2 * max(b, SO.EPS)]
    assert not failures, failures

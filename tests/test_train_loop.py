"""The epoch loop and the command line without a GPU (over the emulator): config ``16``, batch 8, a folder of 24 PNGs at mixed sizes."""
import importlib
import json
import os
import sys

import pytest
import torch

import dataset_cases as DC
from tartangan_amd import backend
from tartangan_amd.trainers.cnn import CNNTrainer
from tartangan_amd.trainers.components import (FIDComponent, ImageSamplerComponent, InfoImageSamplerComponent,
                                               ModelCheckpointComponent)

PER_EPOCH = 3          # 24 images in batches of 8


@pytest.fixture(autouse=True)
def emulated():
    prev = backend._set_backend_for_testing(DC.loop_emulator())
    yield
    backend._set_backend_for_testing(prev)


@pytest.fixture(scope='module')
def folder(tmp_path_factory):
    return DC.write_folder(tmp_path_factory.mktemp('data'), n=24, extras=False)


def _run(argv, seed=5, spy=None):
    tr = CNNTrainer.create_from_cli(argv)
    if spy is not None:
        tr.attach(spy)
    torch.manual_seed(seed)
    import numpy as np
    np.random.seed(seed)
    return tr, tr.train()


def test_event_sequence_counters_and_losses(folder, tmp_path):
    spy = DC.Spy()
    tr, logs = _run(DC.loop_argv(folder, tmp_path, 'r'), spy=spy)
    assert spy.events == DC.expected_events(PER_EPOCH, 2)
    assert (tr.steps, tr.epoch) == (6, 3) and all(len(logs[k]) == 6 for k in ('g_loss', 'd_loss', 'gp'))
    assert [type(c) for c in tr.components] == [ImageSamplerComponent, ModelCheckpointComponent, DC.Spy]
    # bit for bit the hand-written loop from the same seed
    want = DC.hand_driven(CNNTrainer, DC.loop_argv(folder, tmp_path, 'hand'), epochs=2, seed=5)
    assert len(want) == 6
    for i, w in enumerate(want):
        assert {k: logs[k][i] for k in w} == w, i
    root = tmp_path / 'r'
    assert (root / 'samples' / 'sample_0.png').exists() and (root / 'samples' / 'sample_6.png').exists()
    assert json.loads((root / 'checkpoints' / '6' / 'trainer.json').read_text()) == dict(epoch=3, steps=6)


def test_keyboard_interrupt_reaches_train_end_and_checkpoints(folder, tmp_path):
    spy = DC.Spy(interrupt_at=1)
    tr, logs = _run(DC.loop_argv(folder, tmp_path, 'r'), spy=spy)
    assert spy.events[-2][:2] == ('batch_end', 1) and spy.events[-1][:2] == ('train_end', 1)
    assert (tr.steps, tr.epoch) == (1, 1) and len(logs['g_loss']) == 2
    assert (tmp_path / 'r' / 'checkpoints' / '1' / 'g.pt').exists()
    assert json.loads((tmp_path / 'r' / 'checkpoints' / '1' / 'trainer.json').read_text()) == dict(epoch=1, steps=1)


def test_resume_training_latest_continues_where_the_checkpoint_stopped(folder, tmp_path):
    _run(DC.loop_argv(folder, tmp_path, 'r', epochs=1))
    spy = DC.Spy()
    tr, logs = _run(DC.loop_argv(folder, tmp_path, 'r', '--resume-training-latest', epochs=3), spy=spy)
    # the checkpoint of train_end holds epoch 2 / steps 3; the spy is attached last, so it sees the counters as loaded
    assert spy.events[1][:3] == ('epoch_begin', 3, 2)
    assert spy.events[1:] == DC.expected_events(PER_EPOCH, 2, first_step=3, first_epoch=2)[1:]
    assert (tr.steps, tr.epoch) == (9, 4) and len(logs['g_loss']) == 6


def test_cli_flags_file_input_config_and_components(folder, tmp_path):
    argv = [folder, '--batch-size', '8', '--gen-freq', '7', '--lr-g', '2e-4', '--lr-d', '3e-4', '--lr-target-g', '1e-2', '--no-cuda',
            '--epochs', '4', '--output', str(tmp_path), '--dataset-cache', str(tmp_path / 'c' / '{root}_{size}.pkl'), '--grad-penalty', '2',
            '--config', '16', '--model-scale', '1', '--cache-dataset', '--g-base', 'mlp', '--norm', 'bn', '--activation', 'relu',
            '--quiet-logs', '--log-iters', '5', '--log-progress-newlines', '--run-id', 'flags', '--checkpoint-freq', '9',
            '--resume-training-step', 'None']
    tr = CNNTrainer.create_from_cli(argv)
    a = tr.args
    assert (a.data_path, a.batch_size, a.gen_freq, a.lr_g, a.epochs, a.grad_penalty, a.cache_dataset, a.log_iters, a.checkpoint_freq) == \
        (folder, 8, 7, 2e-4, 4, 2., True, 5, 9)
    assert a.quiet_logs and a.log_progress_newlines and a.metrics_collector is None and not a.fid and not a.graphs
    assert a.resume_training_step is None and a.device == 'cpu' and tr.run_id == 'flags'
    assert (tmp_path / 'flags' / 'config.args').read_text().split('\n') == argv
    assert [type(c) for c in tr.components] == [ImageSamplerComponent, ModelCheckpointComponent]
    assert all(c.trainer is tr for c in tr.components)
    # @file: the saved arguments repeat the run; config.args holds the file's lines
    again = CNNTrainer.create_from_cli(['@' + str(tmp_path / 'flags' / 'config.args')])
    assert vars(again.args) == vars(a)
    # a generated run id; --fid adds its component and its flags; 'None' is no run id
    gen = CNNTrainer.create_from_cli([folder, '--no-cuda', '--output', str(tmp_path), '--fid', '--fid-freq', '3', '--run-id', 'None'])
    assert gen.args.run_id and os.path.isdir(tmp_path / gen.args.run_id) and gen.args.fid_freq == 3
    assert [type(c) for c in gen.components] == [ImageSamplerComponent, ModelCheckpointComponent, FIDComponent]
    from tartangan_amd.trainers.info import InfoTrainer
    from tartangan_amd.trainers.text_cnn import TextCNNTrainer
    from tartangan_amd.trainers.components.text_sampler import TextSamplerComponent
    assert InfoTrainer.get_component_classes(a) == [ImageSamplerComponent, ModelCheckpointComponent, InfoImageSamplerComponent]
    assert TextCNNTrainer.get_component_classes(a) == [ModelCheckpointComponent, TextSamplerComponent]


def test_cli_refusals_make_no_run_directory(folder, tmp_path, capsys):
    with pytest.raises(SystemExit, match='metrics-collector tensorboard'):
        CNNTrainer.create_from_cli([folder, '--no-cuda', '--output', str(tmp_path), '--metrics-collector', 'tensorboard'])
    empty = tmp_path / 'empty'
    empty.mkdir()
    for bad in (str(empty), str(tmp_path / 'missing.npz'), __file__):
        with pytest.raises(SystemExit):
            CNNTrainer.create_from_cli([bad, '--no-cuda', '--output', str(tmp_path / 'out')])
    with pytest.raises(SystemExit):
        CNNTrainer.create_from_cli([folder, '--no-cuda', '--output', str(tmp_path / 'out'), '--no-such-flag'])
    assert not (tmp_path / 'out').exists()
    capsys.readouterr()


def test_direct_construction_is_untouched(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    tr = CNNTrainer(CNNTrainer.default_args(config='16', batch_size=8, device='cpu'))
    assert not hasattr(tr.args, 'data_path') and not hasattr(tr.args, 'epochs') and tr.run_id == 'run' and tr.components == []
    assert os.listdir(tmp_path) == []


def test_dataset_cache_flags(folder, tmp_path):
    cache = str(tmp_path / 'cache' / '{root}_{size}.pkl')
    tr, _ = _run(DC.loop_argv(folder, tmp_path, 'r', '--cache-dataset', '--dataset-cache', cache, epochs=1))
    import hashlib
    written = tmp_path / 'cache' / f'{hashlib.md5(folder.encode()).hexdigest()}_16.pkl'
    assert written.exists()

    class NoKernel(type(backend.get())):
        def resample_u8(self, *a):
            raise AssertionError('the dataset cache was not used')
    backend._set_backend_for_testing(NoKernel())
    again, _ = _run(DC.loop_argv(folder, tmp_path, 'r2', '--dataset-cache', cache, epochs=1))
    assert torch.equal(again.dataset.images, tr.dataset.images)
    # an archive instead of a folder: ImageBytesDataset at the model size
    arch, _ = _run(DC.loop_argv(str(written.rename(tmp_path / 'archive.npz')), tmp_path, 'r3', epochs=1))
    assert type(arch.dataset).__name__ == 'ImageBytesDataset' and arch.steps == 3


def test_progress_as_plain_lines(folder, tmp_path, capsys):
    _run(DC.loop_argv(folder, tmp_path, 'r', '--log-progress-newlines', '--log-iters', '2', epochs=1))
    out = capsys.readouterr().out
    assert 'Starting epoch 1' in out and '2/3 [' in out and 'g_loss=' in out and '3/3 [' not in out


@pytest.mark.parametrize('module', ('cnn', 'iqn', 'info', 'scene', 'shared.cnn', 'shared.iqn'))
def test_every_image_trainers_main_runs_an_epoch(module, folder, tmp_path, monkeypatch):
    mod = importlib.import_module('tartangan_amd.trainers.' + module)
    monkeypatch.setattr(sys, 'argv', ['prog'] + DC.loop_argv(folder, tmp_path, 'run', epochs=1))
    torch.manual_seed(0)
    mod.main()
    root = tmp_path / 'run'
    assert (root / 'config.args').exists() and (root / 'samples' / 'sample_3.png').exists()
    assert json.loads((root / 'checkpoints' / '3' / 'trainer.json').read_text()) == dict(epoch=2, steps=3)
    if module == 'info':
        assert (root / 'samples' / 'info_cat_sample_3.png').exists()


def test_the_text_trainers_main_runs_over_a_pickled_frame(tmp_path, monkeypatch):
    import pandas as pd
    from tartangan_amd.trainers import text_cnn
    docs = {'summary': ['the cat sat on the mat. the dog sat too!', 'a bird, a cat and a dog walk in', 'zebra crossing ahead',
                        'the mat sat on the cat', 'a dog and a zebra walk ahead']}
    frame = tmp_path / 'docs.pkl'
    pd.DataFrame(docs).to_pickle(frame)
    monkeypatch.setattr(sys, 'argv', ['prog', str(frame), '--config', '16', '--batch-size', '2', '--epochs', '2', '--no-cuda', '--output',
                                      str(tmp_path), '--run-id', 'text', '--embedding-dims', '8', '--pretrain-embedding', '1', '--quiet-logs'])
    torch.manual_seed(0)
    text_cnn.main()
    root = tmp_path / 'text'
    assert (root / 'samples' / 'sample_4.txt').exists() and (root / 'checkpoints' / '4' / 'trainer.json').exists()
    with pytest.raises(SystemExit):
        monkeypatch.setattr(sys, 'argv', ['prog', str(tmp_path / 'nothing.pkl'), '--no-cuda'])
        text_cnn.main()

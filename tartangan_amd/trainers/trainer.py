"""The reference's ``Trainer`` (trainers/trainer.py) on the HIP engine.

The hot-path half: the latent / batch assembly helpers ``sample_z / sample_g / make_adversarial_batch /
make_generator_batch`` (trainer.py:153-176) and the hyper-parameter flags of the step (trainer.py:268-313).  A tartangan
``Trainer`` can still call ``train_batch(images)`` once per DataLoader batch (trainer.py:96): that call is the drop-in boundary.

The driving half: ``prepare_dataset`` (a folder of images resized on the device, or a uint8 archive), ``train`` -- the reference's
epoch loop (trainer.py:80-115), event for event -- and ``create_from_cli``, the two-stage command line (trainer.py:236-267) with
the reference's flags.  A trainer constructed directly takes no part in any of it: no run id is generated, nothing is written.
"""
import argparse
import hashlib
import os
import random
import string
import sys
import time
from collections import defaultdict
from datetime import datetime

import numpy as np
import torch

from .utils import set_device_from_args

NONE_WORDS = (None, 'None', 'none')


def write_codes(z, cat_dims, cats):
    """The categorical code of InfoGAN latents (trainers/info.py:209-212): columns [0, cat_dims) zeroed, a one at ``cats[row]``."""
    z[:, :cat_dims] = 0.
    z[torch.arange(z.shape[0]), torch.as_tensor(cats, dtype=torch.long)] = 1.
    return z


def _same_numpy_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and tuple(a[2:]) == tuple(b[2:])


class RngFeed:
    """Host-side random inputs of one step (latents z, IQN quantile fractions tau, the scene block's patch noise).

    The reference draws them from the CPU default generator inside the step and moves them
    to the device (trainer.py:153-156, models/iqn.py:105-108).  To replay the step from
    captured HIP graphs the draws have to happen before the launch, into static device
    buffers, in exactly the reference's order.  The first (eager) step records that order;
    afterwards ``refill`` reproduces it.  Under data parallelism every rank draws the GLOBAL
    tensor from the same seed and keeps its own rows (tau rows are quantile-major:
    row = q * B + b), so the union over ranks is the single-process stream.  Kind 'noise' is one (rows, cols) normal draw
    shared by the whole batch (models/blocks/scene.py:139-140): identical on every rank, never sliced.  Kind 'zc' is a latent
    that carries InfoGAN's categorical code in its first ``cat_dims`` columns (trainers/info.py:204-213): a 'z' draw, then one
    ``np.random.randint(0, cat_dims, rows)`` from numpy's GLOBAL generator -- a second host stream -- written as a one-hot row
    by row.  The code is composed on the host, in the staging buffer, so the static device buffer holds the finished latent.
    """

    def __init__(self, device, rank=0, world=1):
        self.device, self.rank, self.world = device, rank, world
        self.plan = []          # [(kind, local_rows, cols)]
        self.static = []
        self.host = []
        self.mode = 'record'
        self.cursor = 0
        self.key = None         # batch shape the plan was recorded for
        self.cat_dims = 0       # width of the categorical code of kind 'zc'
        self.num_items = 0      # vocabulary size of kind 'negatives'
        self._spec = None       # (host generator states before, after) a speculative draw of the next step's inputs
        self._uploaded = None   # event behind the last host -> device copies of the staging buffers
        self._arena = self._host_arena = None   # one allocation behind all of an adopted plan's buffers

    def _draw_cpu(self, kind, rows, cols):
        if kind == 'z':
            full = torch.randn(rows * self.world, cols)
            return full[self.rank * rows:(self.rank + 1) * rows]
        if kind == 'zc':
            full = write_codes(torch.randn(rows * self.world, cols), self.cat_dims,
                               np.random.randint(0, self.cat_dims, rows * self.world))
            return full[self.rank * rows:(self.rank + 1) * rows]
        if kind == 'noise':
            return torch.randn(rows, cols)
        if kind == 'offsets':
            # window offsets of the text trainer (text_cnn.py:168): ``np.random.randint(0, cols, rows)``, numpy's GLOBAL generator
            return torch.from_numpy(np.random.randint(0, cols, rows).astype(np.int64))
        if kind == 'negatives':
            # SkipGram.loss's ``randint_like(context, 0, num_items)`` (models/text.py:50): (rows, cols) int64 below ``self.num_items``
            return torch.randint(0, self.num_items, (rows, cols))
        # tau: (Q*B_global, 1) with row = q*B_global + b  ->  this rank's (Q*B, 1)
        q = cols
        full = torch.rand(rows * self.world, 1)
        b_local = rows // q
        return full.view(q, b_local * self.world)[:, self.rank * b_local:(self.rank + 1) * b_local].reshape(rows, 1)

    def draw(self, kind, rows, cols):
        """kind 'z': (rows, cols) normal;  kind 'tau': (rows, 1) uniform with cols = num_quantiles;  kind 'noise': (rows, cols)
        normal, the same on every rank;  kind 'zc': 'z' with the one-hot categorical code in its first ``cat_dims`` columns;  the
        integer kinds 'offsets' ((rows,) below cols, from numpy) and 'negatives' ((rows, cols) below ``num_items``) are int64 and
        exist for inline drawing only (mode 'off': the text trainer, which does not replay from graphs) -- ``adopt`` / ``refill``
        lay plans out in one float arena and do not take them."""
        if kind in ('offsets', 'negatives') and self.mode != 'off':
            raise NotImplementedError(f"RngFeed kind {kind!r} is drawn inline only (mode 'off')")
        if self.mode == 'off':
            return self._draw_cpu(kind, rows, cols).contiguous().to(self.device)
        if self.mode == 'record':
            val = self._draw_cpu(kind, rows, cols).contiguous()
            buf = val.to(self.device)
            self.plan.append((kind, rows, cols))
            self.static.append(buf)
            host = torch.empty_like(val)
            self.host.append(host.pin_memory() if buf.is_cuda else host)
            return buf
        buf = self.static[self.cursor]          # 'serve'
        assert self.plan[self.cursor] == (kind, rows, cols), 'step structure changed since it was recorded'
        self.cursor += 1
        return buf

    def adopt(self, plan):
        """Start from a plan that is known in advance (the stock trainers' own draw order) instead of recording it during a
        first inline-drawing step: every step, the first included, then has the same structure.

        All of the plan's buffers are slices of ONE device arena (and one pinned staging arena): a step uploads its random
        inputs with a single copy, and the latents lie back to back -- whatever else is drawn between them -- so that the two
        generator passes of a step run over them as one (2B, latent) tensor without joining them first (functional._join)."""
        self.plan = [tuple(p) for p in plan]
        sizes = [rows * (1 if kind == 'tau' else cols) for kind, rows, cols in self.plan]
        order = sorted(range(len(self.plan)), key=lambda i: (self.plan[i][0] not in ('z', 'zc'), i))
        offsets, total = {}, 0
        for i in order:
            offsets[i] = total
            total += (sizes[i] + 3) // 4 * 4                      # 16-byte aligned slices
        self._arena = torch.zeros(max(total, 1), dtype=torch.float32, device=self.device)
        host = torch.zeros(max(total, 1), dtype=torch.float32)
        self._host_arena = host.pin_memory() if self._arena.is_cuda else host
        self.static, self.host = [], []
        for i, (kind, rows, cols) in enumerate(self.plan):
            width = 1 if kind == 'tau' else cols
            self.static.append(self._arena[offsets[i]:offsets[i] + sizes[i]].view(rows, width))
            self.host.append(self._host_arena[offsets[i]:offsets[i] + sizes[i]].view(rows, width))
        self.cursor = 0

    def _draw_into_host(self):
        for (kind, rows, cols), host in zip(self.plan, self.host):
            if self.world == 1:
                # straight into the pinned staging buffer: ``torch.randn(r, c)`` is ``empty(r, c).normal_()`` and
                # ``torch.rand(r, 1)`` is ``empty(r, 1).uniform_()`` -- the same values from the same generator state
                host.uniform_() if kind == 'tau' else host.normal_()
                if kind == 'zc':
                    write_codes(host, self.cat_dims, np.random.randint(0, self.cat_dims, rows))
            else:
                host.copy_(self._draw_cpu(kind, rows, cols))

    def prefetch(self):
        """Draw the NEXT step's inputs while the GPU is busy with this one -- invisibly.  The CPU generator is serial: 63 us per
        (64, 256) latent, and a rank of an N-GPU run draws the GLOBAL tensors (N times that: ~1 ms per step at 8 GPUs), all of
        it GPU idle time if done between a step's loss read-back and the next step's first launch.  So, after a step's work
        has been launched: remember the generator state, draw the plan into the staging buffers, remember the state after,
        and PUT THE GENERATOR BACK.  ``refill`` adopts the values only if the generator is still exactly where it was left
        (then drawing now would produce the same values and end in the remembered state); if anything drew or re-seeded in
        between -- a sampler's ``sample_z(4)``, ``torch.manual_seed`` -- those draws saw the untouched stream, the
        speculation is dropped and the step draws as usual."""
        self._spec = None
        if not self.plan:
            return
        if self._uploaded is not None:
            self._uploaded.synchronize()          # the staging buffers are free (the copies ran at the head of this step)
        before = self._host_streams()
        self._draw_into_host()
        after = self._host_streams()
        self._restore_host_streams(before)
        self._spec = (before, after)

    def _host_streams(self):
        """State of every host generator the plan draws from: torch's, and numpy's global one when a 'zc' entry reads it."""
        uses_numpy = any(kind == 'zc' for kind, _, _ in self.plan)
        return torch.get_rng_state(), (np.random.get_state() if uses_numpy else None)

    @staticmethod
    def _restore_host_streams(state):
        torch.set_rng_state(state[0])
        if state[1] is not None:
            np.random.set_state(state[1])

    def _streams_are_at(self, state):
        now = self._host_streams()
        return torch.equal(now[0], state[0]) and (state[1] is None or _same_numpy_state(now[1], state[1]))

    def refill(self):
        spec, self._spec = self._spec, None
        if spec is not None and self._streams_are_at(spec[0]):       # BOTH streams where the speculation left them
            self._restore_host_streams(spec[1])
        else:
            if self._uploaded is not None:
                self._uploaded.synchronize()
            self._draw_into_host()
        if self._arena is not None:
            self._arena.copy_(self._host_arena, non_blocking=True)       # the whole plan in one upload
        else:
            for buf, host in zip(self.static, self.host):
                buf.copy_(host, non_blocking=True)
        if self.static and self.static[0].is_cuda:
            self._uploaded = torch.cuda.Event()
            self._uploaded.record()
        self.cursor = 0


class Trainer:
    def __init__(self, args, components=()):
        self.args = args
        if not hasattr(args, 'device'):
            set_device_from_args(args)
        self.components = list(components)
        self.steps = 0
        self.epoch = 1
        self.data_parallel = None
        self.rng_feed = RngFeed(self.device)
        self.rng_feed.mode = 'off'
        self._in_step = False        # True only inside train_batch (and graph capture): draws then go through the feed
        sn = getattr(args, 'spectral_norm', 'none')
        if sn not in ('none', 'd', 'g', 'gd'):
            raise ValueError(f'--spectral-norm {sn!r}: one of none, d, g, gd')
        if sn != 'none':
            from .cnn import CNNTrainer
            if type(self) is not CNNTrainer:
                raise NotImplementedError(f'--spectral-norm {sn} is implemented for CNNTrainer only, not for {type(self).__name__}')

    # ------------------------------------------------------------------ hot-path helpers
    @property
    def device(self):
        return self.args.device

    def sample_z(self, n=None):
        """Latents come from the CPU default generator, then move (trainer.py:153-156):
        a seed gives the same z on any device."""
        if n is None:
            n = self.args.batch_size
        return self._draw('z', n, self.gan_config.latent_dims)

    def _draw(self, kind, rows, cols):
        """Random inputs of the step go through ``RngFeed`` (recorded plan, static buffers, per-rank slices).  A draw made
        OUTSIDE a step -- a component's ``sample_z(32)`` at train begin, a user's ``trainer.d(x)`` -- is the reference's
        plain ``torch.randn(n, latent).to(device)`` (trainer.py:153-156) / ``torch.rand(rows, 1)`` (iqn.py:105-108): a fresh
        tensor, never part of the recorded plan, the same values on every rank."""
        if self._in_step:
            return self.rng_feed.draw(kind, rows, cols)
        val = torch.rand(rows, 1) if kind == 'tau' else torch.randn(rows, cols)
        return val.to(self.device)

    def sample_g(self, n=None, target_g=False, **g_kwargs):
        z = self.sample_z(n)
        return (self.target_g if target_g else self.g)(z, **g_kwargs)

    def make_adversarial_batch(self, real_data, **g_kwargs):
        generated = self.sample_g(len(real_data), **g_kwargs)
        batch = torch.cat([real_data, generated], dim=0)
        labels = torch.zeros(len(batch), 1, device=self.device)
        labels[:len(labels) // 2] = 1
        return batch, labels

    def make_generator_batch(self, real_data, **g_kwargs):
        generated = self.sample_g(len(real_data), **g_kwargs)
        return generated, torch.ones(len(generated), 1, device=self.device)

    def build_models(self):
        raise NotImplementedError

    # ------------------------------------------------------------------ what the components read (trainer.py:192-216)
    def get_state(self):
        return dict(epoch=self.epoch, steps=self.steps)

    def set_state(self, state):
        for key, value in state.items():
            setattr(self, key, value)

    @property
    def run_id(self):
        return getattr(self.args, 'run_id', None) or 'run'

    @property
    def output_root(self):
        return f"{getattr(self.args, 'output', './output')}/{self.run_id}"

    def attach(self, *components):
        """Give components their back-reference, like ``ComponentContainer.add_components`` (trainer.py:43-50)."""
        for c in components:
            c.trainer = self
            self.components.append(c)
        return self

    def train_batch(self, imgs):
        raise NotImplementedError

    # ------------------------------------------------------------------ the epoch loop (trainer.py:53-123)
    def prepare_dataset(self):
        """A directory: every image file under it squashed to the model size (``ImageFolderDataset``), from the dataset cache when
        ``--dataset-cache`` names one that exists.  Anything else: a uint8 archive (.npz / .npy), cropped at random to the model size."""
        from ..image_bytes_dataset import ImageBytesDataset
        from ..image_folder_dataset import ImageFolderDataset
        size, path = self.g.max_size, self.args.data_path
        if os.path.isdir(path):
            cache = self.dataset_cache_path(size) if getattr(self.args, 'dataset_cache', None) else None
            return ImageFolderDataset(path, size, device=self.device, cache_path=cache)
        return ImageBytesDataset.from_path(path, crop_size=size, device=self.device)

    def dataset_cache_path(self, size):
        root = getattr(getattr(self, 'dataset', None), 'root', None) or os.path.expanduser(self.args.data_path)
        return self.args.dataset_cache.format(root=hashlib.md5(root.encode('utf-8')).hexdigest(), size=size)

    def batches(self):
        """One epoch of batches -> (iterable, how many).  The order is a ``DataLoader(shuffle=True, drop_last=True)``'s."""
        dp = self.data_parallel
        rank, world = (dp.rank, dp.world) if dp is not None else (0, 1)
        return (self.dataset.loader(self.args.batch_size, rank=rank, world=world),
                len(self.dataset) // (self.args.batch_size * world))

    def invoke(self, event, *args):
        """Every component's ``on_<event>`` hook, in the order the components were attached (components/container.py:14-18)."""
        for component in self.components:
            getattr(component, f'on_{event}')(*args)

    def train(self):
        self.build_models()
        if getattr(self.args, 'graphs', False):
            self.enable_graphs()
        print(f'Preparing dataset from {self.args.data_path}')
        self.dataset = self.prepare_dataset()
        logs = defaultdict(list)
        try:
            self.invoke('train_begin', self.steps, logs)
            while self.epoch <= self.args.epochs:
                print(f'Starting epoch {self.epoch}')
                self.invoke('epoch_begin', self.steps, self.epoch, logs)
                progress = self._progress(*self.batches())
                for images in progress:
                    self.invoke('batch_begin', self.steps, logs)
                    step = self.steps
                    training_metrics = self.train_batch(images)
                    self.steps = step          # train_batch counts its own calls; the loop's count moves after batch_end, as the reference's
                    for name, value in training_metrics.items():
                        logs[name].append(value)
                    self.invoke('batch_end', self.steps, logs)
                    progress.set_postfix(refresh=False, **{k: round(v, 4) for k, v in training_metrics.items()})
                    self.steps += 1
                self.invoke('epoch_end', self.steps, self.epoch, logs)
                if self.epoch == 1 and getattr(self.args, 'cache_dataset', False) and hasattr(self.dataset, 'save_cache'):
                    self.dataset.save_cache(self.dataset_cache_path(self.g.max_size))
                self.epoch += 1
        except KeyboardInterrupt:
            pass          # graceful interrupt
        self.invoke('train_end', self.steps, logs)
        return logs

    def _progress(self, iterable, total):
        """tqdm when it can be imported and ``--log-progress-newlines`` is off, plain lines otherwise; ``--quiet-logs`` reports every
        ``--log-iters`` batches only."""
        args = self.args
        quiet, every = getattr(args, 'quiet_logs', False), getattr(args, 'log_iters', 1000)
        if not getattr(args, 'log_progress_newlines', False):
            try:
                import tqdm
            except ImportError:
                pass
            else:
                return tqdm.tqdm(iterable, total=total, **(dict(mininterval=0, maxinterval=np.inf, miniters=every) if quiet else {}))
        return LineProgress(iterable, total, every if quiet else None)

    # ------------------------------------------------------------------ the command line (trainer.py:218-313)
    @classmethod
    def get_component_classes(cls, args):
        from .components import FIDComponent, ImageSamplerComponent, ModelCheckpointComponent
        collector = getattr(args, 'metrics_collector', None)
        if collector not in NONE_WORDS:
            raise SystemExit(f'--metrics-collector {collector}: the katib / kubeflow / tensorboard writers are not part of '
                             f'tartangan_amd (DESIGN.md section 10); run without the flag')
        classes = [ImageSamplerComponent, ModelCheckpointComponent]
        if getattr(args, 'fid', False):
            classes.append(FIDComponent)
        return classes

    @classmethod
    def _parser(cls, component_classes=()):
        # 'resolve': the samplers bring --gen-freq themselves; the loop's own definition is the same flag
        p = argparse.ArgumentParser(description='TartanGAN trainer', fromfile_prefix_chars='@', conflict_handler='resolve')
        cls.add_args_to_parser(p)
        cls.add_loop_args_to_parser(p)
        for component_class in component_classes:
            component_class.add_args_to_parser(p)
        return p

    @classmethod
    def check_data_path(cls, path):
        """-> why ``path`` cannot be trained from, or None.  Asked before the run directory is made."""
        from ..image_folder_dataset import IMG_EXTENSIONS
        if os.path.isdir(path):
            for _, _, files in os.walk(path):
                if any(os.path.splitext(name)[1] in IMG_EXTENSIONS for name in files):
                    return None
            return f'no image files ({", ".join(IMG_EXTENSIONS)}) under {path}'
        if not os.path.isfile(path):
            return f'{path} does not exist'
        if os.path.splitext(path)[1] not in ('.npz', '.npy'):
            return f'{path} is neither a folder of images nor a uint8 archive (.npz / .npy)'
        return None

    @classmethod
    def create_from_cli(cls, argv=None):
        """Instantiate from the command line (``argv`` default: ``sys.argv[1:]``).  Two stages, as in the reference: the trainer's
        own flags decide which components run, then those add theirs.  The run id, the run directory and its ``config.args`` (the
        arguments, one per line: ``@config.args`` repeats the run) are made here."""
        argv = list(sys.argv[1:] if argv is None else argv)
        base_args = cls._parser().parse_known_args(argv)[0]
        component_classes = cls.get_component_classes(base_args)
        parser = cls._parser(component_classes)
        args = parser.parse_args(argv)
        problem = cls.check_data_path(args.data_path)
        if problem:
            parser.error(problem)
        set_device_from_args(args)
        print(f'Using device "{args.device}"')
        if args.run_id is None:
            args.run_id = generate_run_id()
        trainer = cls(args)
        os.makedirs(trainer.output_root, exist_ok=True)
        save_cli_arguments(f'{trainer.output_root}/config.args', argv)
        return trainer.attach(*[component_class(args) for component_class in component_classes])

    @classmethod
    def add_loop_args_to_parser(cls, p):
        """The reference's flags of the loop (trainer.py:271-313) that ``add_args_to_parser`` -- the flags of the step, which
        ``default_args`` parses with nothing on the line -- leaves out, and ``--graphs``."""
        p.add_argument('data_path', help='A folder of images, or a uint8 image archive (.npz / .npy)')
        p.add_argument('--gen-freq', type=int, default=200, help='Output samples every N batches')
        p.add_argument('--epochs', type=int, default=10000)
        p.add_argument('--output', default='output', help='Root of output locations. A path segment unique to the run will be appended.')
        p.add_argument('--dataset-cache', default='cache/{root}_{size}.pkl', help='Location of the dataset cache of an image folder')
        p.add_argument('--cache-dataset', action='store_true', help='Write the dataset cache after the first epoch')
        p.add_argument('--quiet-logs', action='store_true', help='Reduce log output')
        p.add_argument('--log-iters', type=int, default=1000, help='Progress logging frequency when --quiet-logs are enabled')
        p.add_argument('--log-progress-newlines', action='store_true', help='Log progress updates one per line')
        p.add_argument('--metrics-collector', default=None, help='Not available here (katib, kubeflow, tensorboard in the reference)')
        p.add_argument('--run-id', type=lambda v: None if v in NONE_WORDS else str(v), default=None,
                       help='Explicitly set a run id. Otherwise, one will be generated automatically.')
        p.add_argument('--fid', action='store_true', help='Calculate FID test metric')
        # not in the reference
        p.add_argument('--graphs', action='store_true', help='Replay the step from captured HIP graphs (enable_graphs())')

    # ------------------------------------------------------------------ flags of the step
    @classmethod
    def add_args_to_parser(cls, p):
        p.add_argument('--batch-size', type=int, default=128)
        p.add_argument('--lr-g', type=float, default=1e-4)
        p.add_argument('--lr-d', type=float, default=4e-4)
        p.add_argument('--lr-target-g', type=float, default=1e-3)
        p.add_argument('--no-cuda', action='store_true')
        p.add_argument('--grad-penalty', type=float, default=5.)
        p.add_argument('--config', default='64')
        p.add_argument('--model-scale', type=float, default=1.)
        p.add_argument('--g-base', default='mlp')
        p.add_argument('--norm', default='bn')
        p.add_argument('--activation', default='relu')
        # not in the reference: spectral normalisation of the conv_factory layers of D, G or both
        p.add_argument('--spectral-norm', choices=('none', 'd', 'g', 'gd'), default='none')
        p.add_argument('--spectral-per-layer', action='store_true',
                       help='with --spectral-norm: no spectral scopes, every forward iterates and normalises layer by layer')

    @classmethod
    def default_args(cls, **overrides):
        p = argparse.ArgumentParser()
        cls.add_args_to_parser(p)
        args = p.parse_args([])
        for k, v in overrides.items():
            setattr(args, k, v)
        return args


def generate_run_id(suffix_len=6):
    """``<date>_<time>_<six random letters>`` (trainer.py:205-208)."""
    now = datetime.now().strftime('%Y-%m-%d_%H-%M-%S')
    return f"{now}_{''.join(random.sample(string.ascii_letters, suffix_len))}"


def save_cli_arguments(filename, argv, fromfile_prefix='@'):
    """The arguments, one per line, in a form ``@filename`` reads back; a lone ``@file`` argument is copied out (utils/cli.py:6-23)."""
    lines = list(argv)
    if lines and lines[0].startswith(fromfile_prefix):
        with open(lines[0][1:]) as f:
            lines = [line.strip() for line in f.readlines()] + lines[1:]
    with open(filename, 'w') as f:
        f.write('\n'.join(lines))


class LineProgress:
    """Progress as plain lines: every ``every`` batches, or at most one line a second."""

    def __init__(self, iterable, total, every=None):
        self.iterable, self.total, self.every = iterable, total, every
        self.postfix = {}

    def set_postfix(self, refresh=False, **values):
        self.postfix = values

    def __iter__(self):
        start = last = time.monotonic()
        for i, item in enumerate(self.iterable, 1):
            yield item
            now = time.monotonic()
            if (i % self.every == 0) if self.every else (now - last >= 1.0 or i == self.total):
                last = now
                rate = i / max(now - start, 1e-9)
                print(f'{i}/{self.total} [{rate:.2f}it/s] ' + ', '.join(f'{k}={v}' for k, v in self.postfix.items()), flush=True)

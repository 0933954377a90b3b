"""Text GAN trainer: drop-in for ``tartangan.trainers.text_cnn.TextCNNTrainer`` (reference trainers/text_cnn.py:33-251) on the
HIP engine.

``train_batch(input_indexes) -> {g_loss, d_loss, gp, embedding_loss}`` performs the reference step: one skip-gram step on the two
embedding tables (``tg_skipgram_step``: loss, sparse gradient, SGD at ``--lr-d``), and -- once ``--pretrain-embedding`` batches have
passed -- the D phase (BCE with logits + R1 on the real half) and the G phase over 1-D residual networks that read
``embedding(indexes).permute(0, 2, 1)``, then the EMA of G.  The reference's quirks are kept:

* D gets the same norm as G (text_cnn.py:44) and stays in train mode in the G phase;
* ``update_target_generator`` always uses ``--lr-target-g`` (:237-243), the call in ``build_models`` that passes 1 included, so the
  target is not a copy at start; it also runs during pretraining (:221);
* the returned ``d_loss`` includes the penalty (:205);
* random draws per step, in order: window offsets from numpy's global generator, negatives from torch's CPU generator, the D
  phase's latents, the G phase's latents.

Not available, and refused: HIP-graph replay (``enable_graphs``), data parallelism, attention configs (SelfAttention2d is 2-D).
"""
import numpy as np
import torch

from .. import functional as TF
from ..models.losses import gradient_penalty
from ..models.pluggan import GAN_CONFIGS, Discriminator, Generator
from ..models.text import SkipGram, text_factories
from ..optim import FusedAdam, ema_update
from .cnn import CNNTrainer
from .trainer import Trainer
from .utils import toggle_grad


class TextCNNTrainer(Trainer):
    def build_models(self):
        config = self.args.config
        self.gan_config = GAN_CONFIGS[config] if isinstance(config, str) else config
        self.gan_config = self.gan_config.scale_model(self.args.model_scale)
        self.gan_config = self.gan_config._replace(data_dims=self.args.embedding_dims)
        if self.gan_config.attention:
            raise NotImplementedError('TextCNNTrainer: attention configs are not supported (SelfAttention2d is 2-D)')
        g_kw, d_kw = text_factories(self.args.norm, self.args.activation, self.args.g_base)
        # construction order g, target_g, d consumes the init RNG like the reference (text_cnn.py:85-103)
        self.g = Generator(self.gan_config, **g_kw).to(self.device)
        self.target_g = Generator(self.gan_config, **g_kw).to(self.device)
        self.d = Discriminator(self.gan_config, **d_kw).to(self.device)
        self.optimizer_g = FusedAdam(self.g, lr=self.args.lr_g, betas=(0., 0.999))
        self.optimizer_d = FusedAdam(self.d, lr=self.args.lr_d, betas=(0., 0.999))
        if self.args.activation == 'selu':
            self.init_params_selu(self.g.parameters())
            self.init_params_selu(self.d.parameters())
        self.update_target_generator(1.)     # the reference's "copy weights": moves 1e-3 of the way (see below)
        self.pretraining_embedding = self.args.pretrain_embedding

    init_params_selu = CNNTrainer.init_params_selu

    def build_embedding(self, num_items, padding_idx=0):
        """``SkipGram(len(vocab), embedding_dims, sparse=True, padding_idx=vocab.stoi['<PAD>'])`` of prepare_dataset
        (text_cnn.py:149-156); its optimiser, SGD at --lr-d, is inside ``SkipGram.train_step``."""
        self.embedding = SkipGram(num_items, self.args.embedding_dims, sparse=True, padding_idx=padding_idx).to(self.device)
        self.rng_feed.num_items = num_items
        return self.embedding

    def prepare_dataset(self):
        from ..text_dataset import TextDataset
        self.dataset = TextDataset.from_path(self.args.data_path, doc_len=self.g.max_size)
        self.build_embedding(len(self.dataset.vocab), self.dataset.vocab.stoi['<PAD>'])
        return self.dataset

    def setup_components(self):
        from .components.model_checkpoint import ModelCheckpointComponent
        from .components.text_sampler import TextSamplerComponent
        self.attach(ModelCheckpointComponent(), TextSamplerComponent())

    @classmethod
    def get_component_classes(cls, args):
        """The pair ``setup_components`` attaches (text_cnn.py:128-131), for the command line."""
        from .components.model_checkpoint import ModelCheckpointComponent
        from .components.text_sampler import TextSamplerComponent
        super().get_component_classes(args)          # (refuses a metrics collector)
        return [ModelCheckpointComponent, TextSamplerComponent]

    @classmethod
    def check_data_path(cls, path):
        import os
        return None if os.path.isfile(path) else f'{path} is not a pickled frame of documents'

    def batches(self):
        """The reference's ``DataLoader(dataset, batch_size, shuffle=True, drop_last=True)`` itself (trainer.py:84-86)."""
        from torch.utils.data import DataLoader
        loader = DataLoader(self.dataset, batch_size=self.args.batch_size, shuffle=True, drop_last=True)
        return loader, len(loader)

    # ------------------------------------------------------------------ the step
    def enable_graphs(self):
        raise NotImplementedError('TextCNNTrainer does not replay from HIP graphs (integer draws and the pretraining switch are host-side)')

    def _skipgram_inputs(self, input_indexes):
        """Pivot words, their contexts and the negatives of this batch (text_cnn.py:166-178, models/text.py:50), on the host."""
        context = self.args.context
        window = 2 * context + 1
        offsets = self._draw('offsets', len(input_indexes), window).tolist()
        windows = torch.stack([input_indexes[i, offset:offset + window] for i, offset in enumerate(offsets)])
        words = windows[:, context]
        contexts = torch.cat([windows[:, :context], windows[:, context + 1:]], dim=-1)
        negatives = self._draw('negatives', len(input_indexes), 2 * context)
        return words, contexts, negatives

    def _draw(self, kind, rows, cols):
        if kind in ('offsets', 'negatives'):
            return self.rng_feed._draw_cpu(kind, rows, cols)          # integer kinds stay on the host: they index host data
        return super()._draw(kind, rows, cols)

    def _d_phase(self, inputs):
        toggle_grad(self.g, False)
        toggle_grad(self.d, True)
        self.optimizer_d.zero_grad()
        fake = self.sample_g(len(inputs)).detach()
        real = inputs.detach()
        if self.args.grad_penalty:
            real = real.requires_grad_()
        p_real = self.d(real)
        p_fake = self.d(fake)
        labels = torch.zeros(2 * len(inputs), 1, device=self.device)
        labels[:len(inputs)] = 1
        d_loss = TF.bce_with_logits(torch.cat([p_real, p_fake], dim=0), labels)
        penalty = None
        if self.args.grad_penalty:
            penalty = TF.scale(gradient_penalty(p_real, real), self.args.grad_penalty)
            d_loss = TF.add(d_loss, penalty)
        with TF.grads_into_buckets(), TF.params_only():
            torch.autograd.backward(d_loss, inputs=[p for p in self.d.parameters() if p.requires_grad])
        self.optimizer_d.step()
        return d_loss.detach(), (penalty.detach() if penalty is not None else None)

    def _g_phase(self, batch_size):
        toggle_grad(self.g, True)
        toggle_grad(self.d, False)
        self.optimizer_g.zero_grad()
        fake = self.sample_g(batch_size)
        g_loss = TF.bce_with_logits(self.d(fake), torch.ones(batch_size, 1, device=self.device))
        with TF.grads_into_buckets():
            g_loss.backward()
        self.optimizer_g.step()
        return g_loss.detach()

    def train_batch(self, input_indexes):
        if self.data_parallel is not None:
            raise NotImplementedError('TextCNNTrainer does not run data-parallel (world > 1)')
        if getattr(self, 'embedding', None) is None:
            raise RuntimeError('TextCNNTrainer.train_batch needs the embedding: prepare_dataset() or build_embedding(vocabulary size)')
        input_indexes = torch.as_tensor(np.asarray(input_indexes) if not torch.is_tensor(input_indexes) else input_indexes).long().cpu()
        words, contexts, negatives = self._skipgram_inputs(input_indexes)
        embedding_loss = self.embedding.train_step(words, contexts, negatives, self.args.lr_d)
        self.pretraining_embedding = max(self.pretraining_embedding - 1, 0)
        if not self.pretraining_embedding:
            inputs = self.embedding.gather_t(input_indexes)
            self.g.train()
            self.d.train()
            d_loss, penalty = self._d_phase(inputs)
            g_loss = self._g_phase(len(inputs))
        else:
            g_loss = d_loss = penalty = None
        self.update_target_generator()
        self.steps += 1
        zero = torch.zeros((), device=self.device)
        vals = torch.stack([(v if v is not None else zero).reshape(()).float() for v in (g_loss, d_loss, penalty, embedding_loss)])
        g_loss, d_loss, gp, embedding_loss = vals.tolist()                  # the step's one read-back
        return dict(g_loss=g_loss, d_loss=d_loss, gp=gp, embedding_loss=embedding_loss)

    @torch.no_grad()
    def update_target_generator(self, lr=None):
        """target += (g - target) * lr_target_g; like the reference (text_cnn.py:236-243) ``lr`` is accepted and ignored."""
        ema_update(self.target_g, self.g, self.args.lr_target_g)

    @classmethod
    def add_args_to_parser(cls, p):
        super().add_args_to_parser(p)
        p.add_argument('--embedding-dims', type=int, default=64)
        p.add_argument('--context', type=int, default=3)
        p.add_argument('--pretrain-embedding', type=int, default=10000)


def main():
    TextCNNTrainer.create_from_cli().train()


if __name__ == '__main__':
    main()

"""InfoGAN trainer: drop-in for ``tartangan.trainers.info.InfoTrainer`` (reference trainers/info.py:32-249) on the HIP engine.

The reference's step is the stock CNN step with three additions, and so is this class:

* the discriminator ends in ``MultiModelDiscriminatorOutput`` with two ``LinearOutput`` heads (info.py:65-76): the real / fake
  logit and ``info_cat_dims + info_cont_dims`` code predictions;
* latents carry the codes (info.py:204-213): the first ``info_cat_dims`` columns are a one-hot row drawn from numpy's GLOBAL
  generator (a second host stream next to torch's), the next ``info_cont_dims`` are plain normal columns read back as targets.
  Inside a step they go through ``RngFeed`` kind 'zc', composed on the host, so a step can replay from HIP graphs;
* both phases add ``info_w`` times the code loss -- BCE-with-logits on the categorical columns plus MSE on the continuous ones,
  of D(fake)'s code predictions against the latents that made the fake batch (info.py:139-151, 167-180).  That is ONE launch
  per phase (``functional.info_code_loss``: loss, weighted sum with the adversarial loss, and gradient), reading the targets
  out of the latent buffer in place.  In the paired D pass the code head runs over real | fake like everything else; only the
  fake half's rows are read, and the real half's receive no gradient (info.py:135 discards them).

``train_batch`` returns the reference's five keys from one read-back; the code-loss entries are the unweighted losses.
"""
import functools

import numpy as np
import torch
from torch import nn

from .. import functional as TF
from ..models.blocks import LinearOutput, MultiModelDiscriminatorOutput
from ..models.layers import BatchNorm2d
from ..models.pluggan import Discriminator, Generator
from .cnn import CNNTrainer
from .trainer import write_codes


class InfoTrainer(CNNTrainer):
    d_output_class = MultiModelDiscriminatorOutput
    activations = {k: v for k, v in CNNTrainer.activations.items() if k != 'elu'}      # info.py:45-48 has no 'elu'

    # ------------------------------------------------------------------ model assembly
    def _factories(self):
        f = super()._factories()
        f['d_output'] = functools.partial(
            MultiModelDiscriminatorOutput,
            output_model_factories=[functools.partial(LinearOutput, out_dims=1),
                                    functools.partial(LinearOutput, out_dims=self.args.info_cat_dims + self.args.info_cont_dims)],
            norm_factory={'id': nn.Identity, 'bn': BatchNorm2d}[self.args.norm],
            activation_factory=self.activations[self.args.activation])
        return f

    # ------------------------------------------------------------------ latents
    def z_categorical_code(self, z):
        return z[..., :self.args.info_cat_dims]

    def z_continuous_code(self, z):
        return z[..., self.args.info_cat_dims:self.args.info_cat_dims + self.args.info_cont_dims]

    def _latent_entry(self, bs):
        return ('zc' if self.args.info_cat_dims else 'z', bs, self.gan_config.latent_dims)

    def sample_z(self, n=None):
        """info.py:204-213.  Inside a step the draw goes through ``RngFeed`` (and is remembered: it holds the step's code
        targets); outside one it is the reference's recipe, composed on the host before the move.  Without categorical codes
        numpy's generator is not touched."""
        if n is None:
            n = self.args.batch_size
        cat = self.args.info_cat_dims
        if self._in_step:
            self.rng_feed.cat_dims = cat
            z = self._z_of_phase = self.rng_feed.draw(*self._latent_entry(n))
            return z
        z = torch.randn(n, self.gan_config.latent_dims)
        if cat:
            write_codes(z, cat, np.random.randint(0, cat, (n,)))
        return z.to(self.device)

    def sample_g(self, n=None, target_g=False, **g_kwargs):
        z = self.sample_z(n)
        return (self.target_g if target_g else self.g)(z, **g_kwargs), z

    def make_adversarial_batch(self, real_data, **g_kwargs):
        generated, z = self.sample_g(len(real_data), **g_kwargs)
        batch = torch.cat([real_data, generated], dim=0)
        labels = torch.zeros(len(batch), 1, device=self.device)
        labels[:len(labels) // 2] = 1
        return batch, labels, z

    def make_generator_batch(self, real_data, **g_kwargs):
        generated, z = self.sample_g(len(real_data), **g_kwargs)
        return generated, torch.ones(len(generated), 1, device=self.device), z

    def _sample_fake(self, bs):
        return self.sample_g(bs)[0]

    def _route_rng_through_feed(self):
        super()._route_rng_through_feed()
        self.rng_feed.cat_dims = self.args.info_cat_dims

    def _known_rng_plan(self, bs):
        if type(self) is not InfoTrainer or type(self.g) is not Generator or type(self.d) is not Discriminator:
            return None
        return self._rng_plan(bs)

    # ------------------------------------------------------------------ the step
    def _with_code_loss(self, p_codes, adversarial):
        """-> (unweighted code loss or None, adversarial + info_w * code loss), against the latents of the phase's fake batch
        (``_z_of_phase``: the buffer the generator pass of this phase consumed)."""
        cat, cont = self.args.info_cat_dims, self.args.info_cont_dims
        if not (cat or cont):
            return None, adversarial
        return TF.info_code_loss(p_codes, self._z_of_phase, cat, cont, self.args.info_w, base=adversarial)

    def _d_losses(self, real, fake, labels):
        """info.py:135-151: the adversarial BCE over both halves, the code loss on the fake half alone."""
        if self._d_pairable():
            p_labels, p_codes = self.d(TF.Pair(real, fake))
            p_real, p_codes = p_labels.r, p_codes.f
            adversarial = TF.bce_with_logits(p_labels, labels)
        else:
            p_real, _ = self.d(real)
            p_fake, p_codes = self.d(fake)
            adversarial = TF.bce_with_logits(torch.cat([p_real, p_fake], dim=0), labels)
        self._d_code_loss, d_loss = self._with_code_loss(p_codes, adversarial)
        return p_real, d_loss

    def _g_loss(self, fake, ones):
        p_labels, p_codes = self.d(fake)
        self._g_code_loss, g_loss = self._with_code_loss(p_codes, TF.bce_with_logits(p_labels, ones))
        return g_loss

    def _step_losses(self, g_loss, d_loss, d_grad_penalty):
        return g_loss, d_loss, self._g_code_loss, self._d_code_loss, d_grad_penalty

    def _logs(self, vals):
        codes = 2 if (self.args.info_cat_dims or self.args.info_cont_dims) else 0
        return dict(g_loss=vals[0], g_code_loss=vals[2] if codes else 0., d_loss=vals[1], d_code_loss=vals[3] if codes else 0.,
                    gp=vals[2 + codes] if len(vals) > 2 + codes else 0.)

    def _drop_capture_leftovers(self, labels_before=()):
        super()._drop_capture_leftovers(labels_before)
        for name in ('_z_of_phase', '_d_code_loss', '_g_code_loss'):
            self.__dict__.pop(name, None)

    # ------------------------------------------------------------------ flags
    @classmethod
    def get_component_classes(cls, args):
        from .components import InfoImageSamplerComponent
        return super().get_component_classes(args) + [InfoImageSamplerComponent]      # info.py:107-110

    @classmethod
    def add_args_to_parser(cls, p):
        super().add_args_to_parser(p)
        p.add_argument('--info-cat-dims', type=int, default=10)
        p.add_argument('--info-cont-dims', type=int, default=5)
        p.add_argument('--info-w', type=float, default=1.)


def main():
    InfoTrainer.create_from_cli().train()


if __name__ == '__main__':
    main()

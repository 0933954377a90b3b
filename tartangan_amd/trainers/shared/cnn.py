"""Shared-filter trainer: drop-in for ``tartangan.trainers.shared.cnn.CNNTrainer`` (reference trainers/shared/cnn.py:30-166).

The reference's step is the stock CNN trainer's, statement for statement (BCE-with-logits + R1, Adam(0, .999), the EMA with its
ignored ``lr`` argument); only the models differ: ``SharedGenerator`` / ``SharedDiscriminator`` over the shared-filter blocks.
So this is ``trainers.cnn.CNNTrainer`` with other block factories and model classes.  The bank is one Parameter per network:
it has one slot in the network's FusedAdam bucket, and a data-parallel run all-reduces it with the rest of the bucket.  The
draw order is the stock one (z, z), recorded by the first step as for any subclass; the blocks understand ``Pair``, so the D
phase and the generator's two forwards keep their shared passes.
"""
import functools

from torch import nn

from ...models.layers import BatchNorm2d
from ...models.shared.blocks import SharedResidualDiscriminatorBlock, SharedResidualGeneratorBlock
from ...models.shared.pluggan import SharedDiscriminator, SharedGenerator
from ...models.pluggan import GAN_CONFIGS
from ...optim import FusedAdam
from .. import cnn as _cnn


class CNNTrainer(_cnn.CNNTrainer):
    discriminator_class = SharedDiscriminator

    def _factories(self):
        f = super()._factories()
        bound = dict(norm_factory={'id': nn.Identity, 'bn': BatchNorm2d}[self.args.norm],
                     activation_factory=self.activations[self.args.activation])
        f['g_block'] = functools.partial(SharedResidualGeneratorBlock, **bound)
        f['d_block'] = functools.partial(SharedResidualDiscriminatorBlock, **bound)
        return f

    def build_models(self):
        config = self.args.config
        self.gan_config = GAN_CONFIGS[config] if isinstance(config, str) else config
        self.gan_config = self.gan_config.scale_model(self.args.model_scale)
        f = self._factories()

        def make_g():
            return SharedGenerator(self.gan_config, input_factory=f['g_input'], block_factory=f['g_block'],
                                   output_factory=f['g_output']).to(self.device)
        # construction order g, target_g, d consumes the init RNG like the reference (shared/cnn.py:66-83)
        self.g = make_g()
        self.target_g = make_g()
        self.d = self.discriminator_class(self.gan_config, block_factory=f['d_block'], output_factory=f['d_output']).to(self.device)
        self.optimizer_g = FusedAdam(self.g, lr=self.args.lr_g, betas=(0., 0.999))
        self.optimizer_d = FusedAdam(self.d, lr=self.args.lr_d, betas=(0., 0.999))
        if self.args.activation == 'selu':
            self.init_params_selu(self.g.parameters())
            self.init_params_selu(self.d.parameters())
        self.update_target_generator(1.)


def main():
    CNNTrainer.create_from_cli().train()


if __name__ == '__main__':
    main()

"""Scene trainer: drop-in for ``tartangan.trainers.scene.SceneTrainer`` (reference trainers/scene.py:27-182).

The reference's step is the CNN trainer's, statement for statement (same D, BCE-with-logits + R1, Adam(0, .999), EMA); only
the generator differs: a ``StructuredSceneGenerator`` whose input stage is a ``SceneStructureBlock``.  So this is
``CNNTrainer`` with another generator class and input factory.  The structure block draws one (patch, patch) normal sample per
forward; inside a step that draw goes through ``RngFeed`` (kind 'noise') so that the step's random inputs -- z, noise, z, noise
in the reference's order -- are pre-drawn and the step replays from HIP graphs.  The first step records the draw order
(``_known_rng_plan`` is None for this class) and the generator runs once per phase (``_g_pairable`` is False: each forward
has its own noise).
"""
import functools

from ..models.blocks import SceneStructureBlock
from ..models.pluggan import GAN_CONFIGS, StructuredSceneGenerator
from ..optim import FusedAdam
from .cnn import CNNTrainer


class SceneTrainer(CNNTrainer):
    def build_models(self):
        config = self.args.config
        self.gan_config = GAN_CONFIGS[config] if isinstance(config, str) else config
        self.gan_config = self.gan_config.scale_model(self.args.model_scale)
        f = self._factories()
        g_input = functools.partial(
            SceneStructureBlock, scene_size=self.args.scene_size, patch_size=self.args.patch_size,
            num_patches=self.args.num_patches, refine_patches=self.args.refine_patches, patch_noise=self.args.patch_noise,
            activation_factory=self.activations[self.args.activation])

        def make_g():
            return StructuredSceneGenerator(self.gan_config, input_factory=g_input, block_factory=f['g_block'],
                                            output_factory=f['g_output']).to(self.device)
        # construction order g, target_g, d consumes the init RNG like the reference (scene.py:71-88)
        self.g = make_g()
        self.target_g = make_g()
        self.d = self.discriminator_class(self.gan_config, block_factory=f['d_block'],
                                          output_factory=f['d_output']).to(self.device)
        self.optimizer_g = FusedAdam(self.g, lr=self.args.lr_g, betas=(0., 0.999))
        self.optimizer_d = FusedAdam(self.d, lr=self.args.lr_d, betas=(0., 0.999))
        if self.args.activation == 'selu':
            self.init_params_selu(self.g.parameters())
            self.init_params_selu(self.d.parameters())
        self.update_target_generator(1.)

    def _route_rng_through_feed(self):
        super()._route_rng_through_feed()
        for g in (self.g, self.target_g):
            block = getattr(g, 'structure_generator', None)
            if block is not None and block.noise_source is None:
                block.noise_source = lambda rows, cols: self._draw('noise', rows, cols)

    @classmethod
    def add_args_to_parser(cls, p):
        super().add_args_to_parser(p)
        p.add_argument('--scene-size', type=int, default=16)
        p.add_argument('--patch-size', type=int, default=3)
        p.add_argument('--num-patches', type=int, default=20)
        p.add_argument('--refine-patches', action='store_true')
        p.add_argument('--patch-noise', action='store_true')


def main():
    SceneTrainer.create_from_cli().train()


if __name__ == '__main__':
    main()

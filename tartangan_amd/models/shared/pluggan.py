"""Factory-assembled shared-filter Generator / Discriminator (reference models/shared/pluggan.py:21-123).

A ``SharedModel`` owns ONE filter bank, ``shared_filters[max(blocks), max(latent_dims, *blocks), 3, 3]``, and hands it to every
block it builds; the factories are called with exactly the reference's arguments.  Construction consumes the init RNG like the
reference: the ``randn * 0.01`` draw first, which ``xavier_uniform_`` (gain of 'relu') then overwrites, then the blocks in
order.  ``SharedIQNDiscriminator`` (pluggan.py:126-156) keeps its head outside the Sequential, as ``to_output``, and hands it
the targets; its default head is the fused one (``FusedIQNDiscriminatorOutput``).
"""
import torch
from torch import nn

from ... import functional as TF
from ..blocks import (
    DiscriminatorInput, DiscriminatorOutput, FusedIQNDiscriminatorOutput, GeneratorInputMLP, GeneratorOutput, SelfAttention2d,
)
from .blocks import SharedConvBlock, SharedResidualGeneratorBlock


class SharedModel(nn.Module):
    default_input = GeneratorInputMLP
    default_block = SharedConvBlock
    default_output = GeneratorOutput

    def __init__(self, config, input_factory=None, block_factory=None, output_factory=None):
        super().__init__()
        self.config = config
        self.input_factory = input_factory or self.default_input
        self.block_factory = block_factory or self.default_block
        self.output_factory = output_factory or self.default_output
        max_in_filters = max([config.latent_dims] + list(config.blocks))
        max_out_filters = max(config.blocks)
        filter_size = 3
        self.shared_filters = nn.Parameter(
            torch.randn(max_out_filters, max_in_filters, filter_size, filter_size, requires_grad=True) * 0.01)
        nn.init.xavier_uniform_(self.shared_filters, nn.init.calculate_gain('relu'))
        self.build()

    def build(self):
        raise NotImplementedError

    def forward(self, x):
        # one pass over unchanged weights: each (out, in) view of the bank is materialised once for all its uses.  A scope the
        # caller has open (the trainers bracket a whole phase: several passes and their backward) is used as it is.
        if TF.filter_forms_active():
            return self._run_blocks(x)
        with TF.filter_forms():
            return self._run_blocks(x)

    def _run_blocks(self, x):
        for block in self.blocks:
            x = block(x)
        return x

    @property
    def max_size(self):
        return self.config.base_size * 2 ** len(self.config.blocks)

    def _wants_attention(self, block_i):
        return bool(self.config.attention) and block_i in self.config.attention


class SharedGenerator(SharedModel):
    default_input = GeneratorInputMLP
    default_block = SharedResidualGeneratorBlock
    default_output = GeneratorOutput

    def build(self):
        cfg = self.config
        in_dims = cfg.blocks[0]
        stages = [self.input_factory(cfg.latent_dims, in_dims, cfg.base_size)]
        apply_norm = False
        for block_i, out_dims in enumerate(cfg.blocks):
            stages.append(self.block_factory(self.shared_filters, in_dims, out_dims, apply_norm=apply_norm))
            apply_norm = True
            if self._wants_attention(block_i):
                stages.append(SelfAttention2d(out_dims))
            in_dims = out_dims
        stages.append(self.output_factory(in_dims, cfg.data_dims))
        self.blocks = nn.Sequential(*stages)


class SharedDiscriminator(SharedModel):
    """(The reference's default block here is the GENERATOR block, pluggan.py:96; its trainer always passes the discriminator
    block.  Kept, so that a bare ``SharedDiscriminator(config)`` builds what the reference builds.)"""
    default_input = DiscriminatorInput
    default_block = SharedResidualGeneratorBlock
    default_output = DiscriminatorOutput

    def build(self):
        stages, out_dims = self._stages()
        stages.append(self.output_factory(out_dims, 1))
        self.blocks = nn.Sequential(*stages)

    def _stages(self):
        """-> (from-RGB and the blocks, the width they end at)"""
        cfg = self.config
        in_dims = cfg.blocks[-1]
        stages = [self.input_factory(cfg.data_dims, in_dims)]
        apply_norm = False
        for block_i in reversed(range(len(cfg.blocks))):
            out_dims = cfg.blocks[block_i]
            stages.append(self.block_factory(self.shared_filters, in_dims, out_dims, apply_norm=apply_norm))
            apply_norm = True
            if self._wants_attention(block_i):
                stages.append(SelfAttention2d(out_dims))
            in_dims = out_dims
        return stages, in_dims


class SharedIQNDiscriminator(SharedDiscriminator):
    """pluggan.py:126-156: the blocks in ``self.blocks``, the head beside them as ``self.to_output`` (registered after the blocks,
    like the reference); ``forward(x, targets=None)`` -> ``p_target`` or ``(p_target, loss)``.  A ``Pair`` runs blocks and head
    alike on 2B images; the head draws each half's taus separately, real first."""
    default_output = FusedIQNDiscriminatorOutput

    def build(self):
        stages, out_dims = self._stages()
        self.blocks = nn.Sequential(*stages)
        self.to_output = self.output_factory(out_dims, 1)

    def forward(self, x, targets=None):
        if TF.filter_forms_active():
            return self.to_output(self._run_blocks(x), targets=targets)
        with TF.filter_forms():
            return self.to_output(self._run_blocks(x), targets=targets)

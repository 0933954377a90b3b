"""models/text.py of the reference: the skip-gram embedding of the text trainer, over csrc/text.hip.

``SkipGram`` keeps the reference's constructor, parameters and ``state_dict`` keys (``embedding_u.weight``,
``embedding_v.weight``).  What the reference spreads over ``loss()``, a sparse backward, ``coalesce`` and an SGD optimiser
(trainers/text_cnn.py:162-182) is one call here, ``train_step``: the tables are updated in place by ``tg_skipgram_step`` and the
loss comes back as a device scalar.  ``SkipGram`` builds no autograd graph.

``build_text_models`` assembles the generator and the discriminator over (B, embedding_dims, L) with the factories of the
reference's trainer (trainers/text_cnn.py:34-103), on the 1-D layers of ``models.layers``.  The trainer around them is
``trainers.text_cnn.TextCNNTrainer``."""
import functools

import torch
import torch.nn.functional as F
from torch import nn

from .. import functional as TF
from . import layers as TL
from .blocks import DiscriminatorInput, DiscriminatorOutput, GeneratorInputMLP1d, GeneratorOutput, ResidualDiscriminatorBlock, ResidualGeneratorBlock
from .pluggan import Discriminator, Generator


def text_factories(norm='bn', activation='relu', g_base='mlp', layers=TL):
    """-> (generator factories, discriminator factories) of trainers/text_cnn.py:40-84 as keyword dicts for ``Generator`` /
    ``Discriminator``: the residual blocks with 1-D convolutions, D with the SAME norm as G (the reference's quirk), the block
    shortcut resampled by linear interpolation at scale 0.5, an identity output activation on G.  ``layers``: the namespace the layer
    classes are taken from (``models.layers``; ``torch.nn`` gives the stock modules, for comparisons)."""
    norm_factory = {'id': nn.Identity, 'bn': layers.BatchNorm1d}[norm]
    input_factory = {'mlp': GeneratorInputMLP1d}[g_base]
    activation_factory = {'relu': functools.partial(layers.LeakyReLU, 0.2), 'selu': layers.SELU, 'elu': layers.ELU}[activation]
    half = functools.partial(getattr(layers, 'interpolate', F.interpolate), scale_factor=0.5, mode='linear', align_corners=False)
    g = dict(
        input_factory=functools.partial(input_factory, activation_factory=activation_factory),
        block_factory=functools.partial(ResidualGeneratorBlock, norm_factory=norm_factory, activation_factory=activation_factory,
                                        conv_factory=layers.Conv1d),
        output_factory=functools.partial(GeneratorOutput, norm_factory=norm_factory, activation_factory=activation_factory,
                                         conv_factory=layers.Conv1d, output_activation_factory=nn.Identity))
    d = dict(
        input_factory=functools.partial(DiscriminatorInput, activation_factory=activation_factory, conv_factory=layers.Conv1d),
        block_factory=functools.partial(ResidualDiscriminatorBlock, norm_factory=norm_factory, activation_factory=activation_factory,
                                        conv_factory=layers.Conv1d, avg_pool_factory=layers.AvgPool1d, interpolate=half),
        output_factory=functools.partial(DiscriminatorOutput, norm_factory=norm_factory, activation_factory=activation_factory))
    return g, d


def build_text_models(config, norm='bn', activation='relu', g_base='mlp', layers=TL):
    """-> (Generator, Discriminator) over (B, embedding_dims, L) as trainers/text_cnn.py:85-103 assembles them;
    ``config.data_dims`` is the embedding width."""
    if config.attention:
        raise NotImplementedError('the text models have no attention: SelfAttention2d is 2-D')
    g, d = text_factories(norm, activation, g_base, layers)
    return Generator(config, **g), Discriminator(config, **d)


class SkipGram(nn.Module):
    def __init__(self, num_items, item_dims, **embedding_kwargs):
        super().__init__()
        self.embedding_u = nn.Embedding(num_items, item_dims, **embedding_kwargs)
        self.embedding_v = nn.Embedding(num_items, item_dims, **embedding_kwargs)
        self.num_items = num_items

    @property
    def padding_idx(self):
        return self.embedding_u.padding_idx

    def forward(self, x):
        """embedding_u(x), (..., E); no gradient (the reference's only caller detaches it)."""
        shape = tuple(x.shape)
        return self.gather_t(x.reshape(1, -1))[0].t().reshape(*shape, -1)

    def gather_t(self, indexes):
        """embedding_u(indexes).permute(0, 2, 1) for (B, L) indexes, as the contiguous (B, E, L) tensor the discriminator takes."""
        return TF.embed_gather_t(self.embedding_u.weight, indexes)

    def draw_negatives(self, contexts):
        """The reference's ``torch.randint_like(context, 0, num_items)`` from the CPU generator (the same stream for a CPU context)."""
        return torch.randint(0, self.num_items, tuple(contexts.shape))

    def train_step(self, words, contexts, negatives=None, lr=0.0):
        """loss(words, contexts) of the tables as they are, then plain SGD at ``lr`` on both, in place.  -> the loss, a device scalar."""
        if negatives is None:
            negatives = self.draw_negatives(contexts)
        return TF.skipgram_step(self.embedding_u.weight.data, self.embedding_v.weight.data, words, contexts, negatives, lr, self.padding_idx)

    def lookup(self, zs):
        """Nearest row of embedding_u for each column of zs (batch, embedding_dims, steps): a list of (steps,) index tensors that
        skip row 0 and count from row 1, exactly as the reference returns them."""
        return list(TF.embed_lookup(self.embedding_u.weight, zs))

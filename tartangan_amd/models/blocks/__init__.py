from .attention import SelfAttention2d  # noqa
from .discriminator import (  # noqa
    DiscriminatorInput, DiscriminatorOutput, FusedIQNDiscriminatorOutput, IQNDiscriminatorOutput, LinearOutput, MultiModelDiscriminatorOutput,
    ResidualDiscriminatorBlock,
)
from .generator import (  # noqa
    GeneratorInputMLP, GeneratorInputMLP1d, GeneratorOutput, ResidualGeneratorBlock, TiledZGeneratorInput,
)
from .scene import SceneStructureBlock  # noqa

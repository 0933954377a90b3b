"""Trainer components of the reference that a run behind the drop-in needs next to the step:
checkpoint / resume, the progress sampler and the InfoGAN trainer's code sweeps.  Same class names, hooks and file layout as
``tartangan.trainers.components``; a tartangan ``Trainer`` can attach either family."""
from .base import TrainerComponent
from .image_sampler import ImageSamplerComponent
from .info_image_sampler import InfoImageSamplerComponent
from .model_checkpoint import ModelCheckpointComponent
from .metrics import FIDComponent

__all__ = ['TrainerComponent', 'ImageSamplerComponent', 'InfoImageSamplerComponent', 'ModelCheckpointComponent', 'FIDComponent']

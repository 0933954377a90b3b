"""Shared-filter IQN trainer: drop-in for ``tartangan.trainers.shared.iqn.IQNTrainer`` (reference trainers/shared/iqn.py:31-153).

The shared CNN trainer's models (``SharedGenerator``, the shared-filter blocks, one bank per network) with the IQN trainer's
step: the discriminator is a ``SharedIQNDiscriminator`` whose head returns ``(p_target, loss)``, ``d_loss = loss_real +
loss_fake``, R1 on the quantile-mean prediction, ``g_loss`` the head's loss against all-ones targets.  The draw order is
z, taus of D(real), taus of D(fake), z, taus of the G phase's D(fake), recorded by the first step as for any subclass.

The head is the fused one (``FusedIQNDiscriminatorOutput``: one launch each way behind the pooled features).  One quirk of the
reference is kept: it builds a ``d_output_factory`` bound to ``--norm`` and ``--activation`` and then passes the bare
``IQNDiscriminatorOutput`` class (shared/iqn.py:63-66, 80-84), so the head is BatchNorm2d + LeakyReLU(0.2) whatever the flags say.
``init_params_selu`` still runs over all of the discriminator's parameters under ``--activation selu``.
"""
from ...models.blocks import FusedIQNDiscriminatorOutput
from ...models.shared.pluggan import SharedIQNDiscriminator
from .. import iqn as _iqn
from .cnn import CNNTrainer


class IQNTrainer(CNNTrainer):
    discriminator_class = SharedIQNDiscriminator
    d_output_class = FusedIQNDiscriminatorOutput
    activations = {k: v for k, v in CNNTrainer.activations.items() if k in ('relu', 'selu')}      # shared/iqn.py:43-46

    def _factories(self):
        f = super()._factories()
        f['d_output'] = self.d_output_class          # the bare class: the reference drops the bound norm / activation (:83)
        return f

    _d_losses = _iqn.IQNTrainer._d_losses
    _rng_plan = _iqn.IQNTrainer._rng_plan
    _g_loss = _iqn.IQNTrainer._g_loss


def main():
    IQNTrainer.create_from_cli().train()


if __name__ == '__main__':
    main()

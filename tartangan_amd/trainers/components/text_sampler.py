"""Text progress samples (reference components/text_sampler.py:13-49) for the HIP text trainer.

``sample_z(32)`` is drawn when training begins; an output runs ``g`` on those latents under ``no_grad`` in whatever mode it is in,
takes the first 16 documents, finds the nearest word of every column with ``SkipGram.lookup`` and decodes the indexes with
``vocab.itos`` EXACTLY as the reference does -- its lookup skips row 0 and counts from row 1, so index i prints ``itos[i]``, one word
off the row that actually won; that is the reference's behaviour and is kept.  Documents are wrapped at 70 columns and separated by
a line of 40 dashes."""
import os
import textwrap

import torch

from .base import TrainerComponent


class TextSamplerComponent(TrainerComponent):
    def on_train_begin(self, steps, logs):
        os.makedirs(self.sample_root, exist_ok=True)
        self.progress_samples = self.trainer.sample_z(32)

    def on_train_end(self, steps, logs):
        self.output_samples(f'{self.sample_root}/sample_{steps}.txt')

    def on_batch_end(self, steps, logs):
        if steps % self.trainer.args.gen_freq == 0:
            self.output_samples(f'{self.sample_root}/sample_{steps}.txt')

    def output_samples(self, filename, n=None):
        with torch.no_grad():
            generated = self.trainer.g(self.progress_samples)[:16]
            generated = self.trainer.embedding.lookup(generated)
            v = self.trainer.dataset.vocab
            with open(filename, 'w') as outfile:
                for result in generated:
                    doc = ' '.join(v.itos[i] for i in result.tolist())
                    outfile.writelines([s + '\n' for s in textwrap.wrap(doc, 70)])
                    outfile.write('-' * 40 + '\n')

    @property
    def sample_root(self):
        return f'{self.trainer.output_root}/samples'

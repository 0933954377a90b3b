"""text_dataset.py of the reference without torchtext: documents as fixed-length rows of vocabulary indexes.

The reference builds its tokenizer and vocabulary with ``torchtext.data.utils.get_tokenizer('basic_english')`` and the legacy
``torchtext.vocab.Vocab(counter, specials=['<unk>', '<pad>'])``.  Both are small and are written out here, so the package does not
need torchtext:

* ``basic_english``: lower-case, put spaces around ``' . , ( ) ! ?``, drop ``"``, turn ``; :`` and ``<br />`` into a space, split on
  white space;
* ``Vocab``: ``itos`` = the specials in the order given, then every word by falling count, equal counts alphabetically; ``stoi`` maps
  a key it does not know to index 0 (``<unk>``).  The reference's trainer asks for ``stoi['<PAD>']`` (upper case, not a special), so
  its ``padding_idx`` is 0 -- the same 0 that ``np.pad`` fills short documents with.

Tokenizer and vocabulary order were written from the documented behaviour of those two torchtext pieces; they could not be compared
with torchtext itself where this was developed."""
import collections
import re

import numpy as np
from torch.utils.data import Dataset

_BASIC_ENGLISH = [(re.compile(p), r) for p, r in (
    (r"\'", " '  "), (r'\"', ''), (r'\.', ' . '), (r'<br \/>', ' '), (r',', ' , '), (r'\(', ' ( '), (r'\)', ' ) '), (r'\!', ' ! '),
    (r'\?', ' ? '), (r'\;', ' '), (r'\:', ' '), (r'\s+', ' '))]


def basic_english(line):
    line = line.lower()
    for pattern, replacement in _BASIC_ENGLISH:
        line = pattern.sub(replacement, line)
    return line.split()


def get_tokenizer(name):
    if callable(name):
        return name
    if name == 'basic_english':
        return basic_english
    if name is None:
        return str.split
    raise NotImplementedError(f'tokenizer {name!r}: basic_english, None (white space) or a callable')


class _Stoi(collections.defaultdict):
    """word -> index; a key that is not in the vocabulary reads as 0 and is not added."""

    def __missing__(self, key):
        return 0


class Vocab:
    def __init__(self, counter, specials=('<unk>', '<pad>'), min_freq=1):
        self.freqs = counter
        self.itos = list(specials)
        words = sorted((w for w in counter if w not in specials), key=lambda w: (-counter[w], w))
        self.itos += [w for w in words if counter[w] >= max(min_freq, 1)]
        self.stoi = _Stoi()
        self.stoi.update({w: i for i, w in enumerate(self.itos)})

    def __len__(self):
        return len(self.itos)


class TextDataset(Dataset):
    """``df_docs``: a pandas DataFrame (as the reference pickles it) or any mapping from column name to a sequence of strings."""

    def __init__(self, df_docs, doc_len=128, transform=None, column='summary', tokenizer='basic_english'):
        super().__init__()
        self.df_docs = df_docs
        self.doc_len = doc_len
        self.column = column
        self.transform = transform
        self.tokenizer = get_tokenizer(tokenizer)
        self.build_vocab()

    def build_vocab(self):
        tokenized = [self.tokenizer(doc) for doc in self.df_docs[self.column]]
        frequencies = collections.Counter()
        for tokens in tokenized:
            frequencies.update(tokens)
        self.vocab = Vocab(frequencies, specials=['<unk>', '<pad>'])
        self.doc_indexes = [[self.vocab.stoi[t] for t in tokens] for tokens in tokenized]

    def __getitem__(self, idx):
        indexes = self.doc_indexes[idx]
        if len(indexes) < self.doc_len:
            return np.pad(np.asarray(indexes, dtype=np.int64), (0, self.doc_len - len(indexes)), 'constant')
        return np.array(indexes[:self.doc_len], dtype=np.int64)

    def __len__(self):
        return len(self.doc_indexes)

    @classmethod
    def from_path(cls, path, **cls_kwargs):
        import pandas as pd
        with open(path, 'rb') as infile:
            docs = pd.read_pickle(infile, compression=None)
        return cls(docs, **cls_kwargs)

"""The LDS-DMA rule of test_source_rules.py applied to csrc/inception.hip: any `dma16` call there sits under wave-uniform
conditions only.  (The file stages global -> registers -> LDS and has no LDS-DMA today; this keeps it honest if one arrives.)"""
import os
import re

from test_source_rules import HERE, SCALAR_TOKEN, _guards

INCEPTION = os.path.join(os.path.dirname(HERE), 'tartangan_amd', 'csrc', 'inception.hip')


def test_inception_lds_dma_sites_are_wave_uniform():
    for lineno, cond, stmt in _guards(INCEPTION):
        assert cond is not None, f'inception.hip line {lineno}: unguarded or unparsable dma16 call: {stmt}'
        for tok in re.findall(r'[A-Za-z_]\w*|\d+', cond):
            assert SCALAR_TOKEN.match(tok), f'inception.hip line {lineno}: `{tok}` in the guard of an LDS-DMA is not wave-uniform'


def test_inception_wave_index_is_scalar():
    src = open(INCEPTION).read()
    assert re.search(r'\bwave\s*=\s*__builtin_amdgcn_readfirstlane\(', src)    # which k rows a wave gathers must be wave-uniform
    assert 'atomic' not in src.lower().replace('no atomics', '')            # fixed-order sums only

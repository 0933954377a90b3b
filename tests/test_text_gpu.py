"""The text trainer on the GPU: ``trainers.text_cnn.TextCNNTrainer`` against the three fixtures recorded from the reference's own
trainer (tests/golden/text_*.json, made by tests/golden/make_text_golden.py), every loss and norm of every step within 1e-4; the same
step twice from the same state bit-equal; and the 1-D generator and discriminator with an R1 step against float64 stock layers
(bound 1e-4 relative to the largest reference value, the bound of every whole-network quantity of this repository's fixtures)."""
import numpy as np
import pytest
import torch

import test_text
import text_cases as TC

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def hip_backend():
    from tartangan_amd import backend
    prev = backend._set_backend_for_testing(None)
    backend.get()
    yield
    backend._set_backend_for_testing(prev)


@pytest.mark.parametrize('case', TC.TEXT_CASES)
def test_trainer_against_the_reference_fixtures(case):
    test_text.check_trainer_against_fixture(case, 'cuda')


@pytest.mark.parametrize('case', ['text_c16_e8_b4', 'text_c32_e16_b4_id'])
def test_the_same_steps_twice_from_the_same_state_are_bit_equal(case):
    fx = TC.load_text_fixture(case)
    runs = []
    for _ in range(2):
        tr, entries = test_text.run_fixture_steps(fx, 'cuda')
        state = [t.detach().reshape(-1).float() for m in (tr.g, tr.d, tr.target_g, tr.embedding) for t in m.state_dict().values()]
        runs.append((entries, torch.cat(state).cpu().view(torch.int32)))
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1])


def test_generator_discriminator_and_the_r1_step_against_float64_stock_layers():
    test_text.check_text_models('cuda', torch.float32, 1e-4)

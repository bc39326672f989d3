"""The text stack issues the recorded kernel-library calls, call for call: every case of tests/golden/make_text_stack_launches.py
(encode / encode_cls / DecoderSession / score / start_logits / the HF-signature forwards, both LayerNorm schedules, image blocks,
more than LONG_KEYS encoder states, the parity mode in each attention kind, the sentence encoder) through that file's recorder,
against tests/golden/text_stack_launches.json.xz.  A trace holds, per call, the function, every scalar by value and every tensor's
dtype, shape, strides, storage offset and storage ordinal — equal traces are the same kernels on the same operands with the same
aliasing.  After a deliberate change of the launch sequence the golden is recorded again with that file."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_text_stack_launches as rec  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = rec.cases()


@pytest.fixture(scope="module")
def models():
    return rec.Models()


@pytest.fixture(scope="module")
def golden():
    return rec.load_golden()


def test_the_golden_holds_exactly_the_cases(golden):
    assert sorted(golden) == sorted(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_launches_equal_the_recorded_ones(name, models, golden):
    got, want = rec.trace(CASES[name], models), golden[name]
    for n, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{name}: call {n} differs"
    assert len(got) == len(want), f"{name}: {len(got)} calls, {len(want)} recorded"

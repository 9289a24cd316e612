"""The four windowed diagnostics against the bits they gave before the code they share moved to csrc/diag_common.hpp
(tests/golden/diag_bits.json, written by the library of the commit before: tests/golden/make_diag_bits.py).  The cases, their
inputs and the raw calls are tests/diag_dev.py's.  There is no tolerance: every count is an integer and every sum has a fixed
order, so the same operations give the same bits."""
import functools
import json
import os

import pytest

from diag_dev import CASES, run_case
from gelman_dev import bit_checksums

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def fixture():
    return json.load(open(os.path.join(os.path.dirname(__file__), "golden", "diag_bits.json")))


def test_the_fixture_holds_every_case():
    assert sorted(fixture()) == sorted(CASES)


@pytest.mark.parametrize("key", list(CASES))
def test_the_diagnostics_give_the_bits_of_the_parent(key):
    assert {name: bit_checksums(v) for name, v in run_case(key).items()} == fixture()[key]

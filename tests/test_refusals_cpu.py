"""The rows of tests/refusals.py that need no device, on host tensors: the scalar and int rules, which fire before any tensor is
looked at, and the form parsers of flownet, which touch no device."""
import pytest

import refusals


@pytest.mark.parametrize('op_row', refusals.CPU_ROWS, ids=refusals.row_id)
def test_refused_without_a_device(op_row):
    assert refusals.verdict(op_row[0], op_row[1], 'cpu') is None

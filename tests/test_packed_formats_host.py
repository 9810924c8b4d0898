"""CPU: the table of packed-row formats (``ops.PACKED_FORMATS``) agrees with the C ABI (``_lib.SIGNATURES``, include/allset_hip_ext.h), and
a format is never defaulted: everything that takes one refuses a missing or an unknown name."""
import inspect
import os
import re

import pytest
import torch

from allset_amd import _lib, dense, ops
from allset_amd import functional as AF

HEADER_EXT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "allset_hip_ext.h")
CAP_CONSTANT = {"mask": "kPackCap", "cells": "kCellCap"}
FORMATS = sorted(ops.PACKED_FORMATS)


def test_the_table_holds_the_two_formats():
    assert FORMATS == sorted(CAP_CONSTANT)


@pytest.mark.parametrize("fmt", FORMATS)
def test_symbols_are_declared(fmt):
    entry = ops.PACKED_FORMATS[fmt]
    for role in ("pack", "gather", "linear", "supported"):
        assert entry[role] in _lib.SIGNATURES, (fmt, role)


@pytest.mark.parametrize("fmt", FORMATS)
def test_signatures_have_the_other_formats_arity(fmt):
    entry = ops.PACKED_FORMATS[fmt]
    for other in FORMATS:
        for role in ("pack", "gather", "linear"):
            assert len(_lib.SIGNATURES[entry[role]]) == len(_lib.SIGNATURES[ops.PACKED_FORMATS[other][role]]), (fmt, other, role)


@pytest.mark.parametrize("fmt", FORMATS)
def test_capacity_is_the_headers(fmt):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER_EXT).read(), flags=re.S)
    m = re.search(r"\b%s\s*=\s*(\d+)" % CAP_CONSTANT[fmt], text)
    assert m is not None, CAP_CONSTANT[fmt]
    assert ops.PACKED_FORMATS[fmt]["cap"] == int(m.group(1))


def test_packed_rows_takes_no_default_format():
    t = torch.zeros(1)
    with pytest.raises(TypeError):
        dense.PackedRows(t, t)
    for fmt in FORMATS:
        assert dense.PackedRows(t, t, fmt).format == fmt


def test_an_unknown_format_is_a_value_error():
    t = torch.zeros(1)
    with pytest.raises(ValueError):
        dense.PackedRows(t, t, "rows")
    before = {d: AF.packed_format(d) for d in ("v2e", "e2v")}
    with pytest.raises(ValueError):
        AF.set_packed_format("rows")
    assert {d: AF.packed_format(d) for d in ("v2e", "e2v")} == before


@pytest.mark.parametrize("op", [ops.pack_rows, ops.segreduce_packed, ops.fused_linear_fwd_packed, ops.fused_linear_fwd_packed_supported])
def test_ops_require_fmt_by_keyword(op):
    p = inspect.signature(op).parameters["fmt"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is inspect.Parameter.empty

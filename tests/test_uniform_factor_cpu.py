"""RMA_DIAG uniform_factor (the 1/Cp field path also where 1/Cp is one value):
the key parses on both sides and is documented; the tuning field that asks a
K-step launch for the uniform-factor kernel is a trailing, default-off field."""
import dataclasses
import os

import pytest

from rocm_mpi_amd import config, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_uniform_factor_key_parses_and_is_documented():
    assert "uniform_factor" in config.DIAG_KEYS
    assert config.diag_entries("uniform_factor=off") == {"uniform_factor": "off"}
    assert config.diag_entries("no_lag,uniform_factor=off")["uniform_factor"] == "off"
    with pytest.raises(Exception):
        config.diag_entries("uniform_factors=off")
    doc = open(os.path.join(ROOT, "docs", "TUNING.md")).read()
    assert "`uniform_factor=off`" in doc
    src = open(os.path.join(ROOT, "csrc", "runtime", "config.cpp")).read()
    assert '"uniform_factor",' in src


def test_native_side_accepts_the_key(monkeypatch):
    from rocm_mpi_amd._native import native

    monkeypatch.setenv("RMA_DIAG", "uniform_factor=off")
    assert native().diag_value("uniform_factor") == "off"


def test_tuning_field_is_trailing_and_off_by_default():
    names = [f.name for f in dataclasses.fields(ops.StencilTuning)]
    assert names[-2:] == ["uniform", "uniform_value"] and names[-3] == "cols"
    assert ops.StencilTuning().uniform is False and ops.StencilTuning().uniform_value is None

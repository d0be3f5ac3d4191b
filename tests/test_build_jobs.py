"""build.py compiles its stale sources in parallel: MAX_JOBS bounds the compilers where it is set, and 16 bounds them always (a shared
build machine shows far more CPUs than a build may use)."""
import os

import pytest

from lfr_amd import build


@pytest.mark.parametrize("env, cpus, want", [("4", 64, 4), ("64", 64, 16), (None, 8, 8), (None, 192, 16), ("0", 8, 1), ("many", 8, 8)])
def test_jobs_honour_max_jobs_and_the_cap(monkeypatch, env, cpus, want):
    if env is None: monkeypatch.delenv("MAX_JOBS", raising=False)
    else: monkeypatch.setenv("MAX_JOBS", env)
    monkeypatch.setattr(os, "cpu_count", lambda: cpus)
    assert build._jobs() == want

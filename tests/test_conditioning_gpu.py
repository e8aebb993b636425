"""What a call runs beside the UNet is resolved in one place (model.hip resolve_cond: the set states, one conflict table, the fit checks).
tests/golden/conditioning_parent.npz holds what commit 00fefd3 -- one helper per feature -- refused, computed and launched in the cases of
tools/record_conditioning.py, recorded on one MI355X (two runs there were identical; csrc/ has no atomics).  The same cases replayed on this
build must give the same message strings, the same latents / eps bit for bit and the same launches per kernel class."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def recorder():
    spec = importlib.util.spec_from_file_location("record_conditioning", os.path.join(ROOT, "tools", "record_conditioning.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def parent(golden_dir):
    return np.load(os.path.join(golden_dir, "conditioning_parent.npz"))


@pytest.fixture(scope="module")
def now(recorder):
    """Every case on this build, run once and left unchanged."""
    return recorder.record()


def _names(rec, kind):
    return sorted(k for k in (rec.files if hasattr(rec, "files") else rec) if k.startswith(kind + "/"))


def test_the_replay_runs_the_recorded_cases(now, parent):
    assert sorted(now) == sorted(parent.files)
    assert len(_names(parent, "refusal")) > 100 and len(_names(parent, "out")) >= 20
    assert list(now["classes"]) == list(parent["classes"])


def test_refusals_are_the_parents(now, parent):
    """String equality, a call that runs being ""; which refusal wins where two states are set is part of the string."""
    bad = {k: (str(now[k]), str(parent[k])) for k in _names(parent, "refusal") if str(now[k]) != str(parent[k])}
    assert not bad, bad


def test_outputs_are_the_parents_bit_for_bit(now, parent):
    for k in _names(parent, "out"):
        want, got = torch.from_numpy(parent[k]), torch.from_numpy(now[k])
        assert want.dtype == torch.float32 and torch.isfinite(want).all(), k
        assert torch.equal(got, want), (k, float((got - want).abs().max()))
    # the conditioned cases are not the plain one: each recorded state did run
    plain = parent["out/e4/denoise/plain"]
    for s in ("cn", "gl", "cn+gl", "ad", "ipa", "inp", "inp+gl"):
        assert not np.array_equal(parent["out/e4/denoise/" + s], plain), s


def test_launch_counts_are_the_parents(now, parent):
    for k in _names(parent, "launches"):
        assert parent[k].sum() > 0, k
        assert np.array_equal(now[k], parent[k]), (k, dict(zip(parent["classes"], zip(now[k], parent[k]))))


def test_every_cell_of_the_conflict_table_is_refused_somewhere(parent):
    """The non-null cells of kConflicts are its string literals, read from the source and counted there: each is the tail of at least
    one recorded message, so no pair the table refuses went unrecorded -- and the recording, being the parent's, had it refused already."""
    src = open(os.path.join(ROOT, "agenda_amd", "csrc", "model.hip")).read()
    table = src[src.index("static const ConflictRow kConflicts[] = {"):]
    table = table[:table.index("\n};")]
    rows = table.count("{ ST_") + table.count("{ -1,")
    cells = re.findall(r'"((?:[^"\\]|\\.)*)"', table)
    nulls = len(re.findall(r"\bnullptr\b", table))
    assert rows == 6 and len(cells) + nulls == rows * 6 and len(set(cells)) == len(cells)
    said = [str(parent[k]) for k in _names(parent, "refusal")]
    hit = [c for c in cells if any(m.endswith(c) for m in said)]
    assert len(hit) == len(cells), sorted(set(cells) - set(hit))

"""fountain_amd.render's command line against what it answered before its refusals became one table and one function: every single
option group, every pair and triple of them, under --gpus 1 and under a launcher, the bad values, the refusals that need the parsed
scene, the names of the files beside the image, and (on the GPU) the files three renders write.  The lines and the recorder are
tests/_render_cli_cases.py; the recordings are tests/golden/render_cli_refusals.json and render_cli_outputs.json."""
import itertools
import json
import os
import subprocess
import sys

import pytest

import _render_cli_cases as K

ROOT = K.ROOT


@pytest.fixture(scope="module")
def rec():
    return json.load(open(K.REFUSALS))


def _same(got, want):
    bad = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not bad and got.keys() == want.keys(), bad


def test_singles_and_pairs(rec):
    """exit code and stderr byte for byte; a line that went on to the library or to starting ranks still does, and no other"""
    _same(K.answers(K.singles_and_pairs()), rec["lines"])
    kinds = [v if isinstance(v, str) else "refused" for v in rec["lines"].values()]
    assert (kinds.count("refused"), kinds.count("ranks"), kinds.count("library")) == (160, 2, 48)


def test_gpus_1(rec):
    """`--gpus 1` is "given" to the first-hit, denoise and variance options and to --compare-to, and not to --png, --adaptive, --pixel-filter"""
    assert len(rec["gpus_1"]) == 20
    _same(K.answers(K.with_gpus_1()), rec["gpus_1"])


def test_under_a_launcher(rec, monkeypatch):
    for k, v in K.WORLD.items():
        monkeypatch.setenv(k, v)
    assert len(rec["launcher"]) == 21
    _same(K.answers([[]] + K.combos(1)), rec["launcher"])


def test_bad_values(rec):
    assert len(rec["bad_values"]) == len(K.BAD_VALUES)
    _same(K.answers(K.BAD_VALUES), rec["bad_values"])


def test_triples(rec):
    """Where three options conflict, which applicable message comes first may follow the table's order: the exit code is the
    recording's, and the message is one that a single or a pair out of the triple gets.  A triple that went on still does."""
    got = K.answers(K.combos(3))
    assert len(got) == 1140
    for groups in itertools.combinations(K.GROUPS, 3):
        k = K.key(sum(groups, []))
        if isinstance(rec["triples"][k], str):
            assert got[k] == rec["triples"][k], k
            continue
        allowed = K.triple_messages(rec, groups)
        assert allowed and got[k][0] == rec["triples"][k] == 2 and got[k][1] in allowed, (k, got[k], allowed)


def test_scene_dependent_refusals(rec, ftn, tmp_path, monkeypatch):
    """the four checks that need the parsed scene come before a scene is created, and nothing is written"""
    from fountain_amd.api import PbrtScene
    monkeypatch.setattr(PbrtScene, "create_scene", lambda *a, **k: pytest.fail("a scene was created before the refusal"))
    refs, work = tmp_path / "refs", tmp_path / "work"
    refs.mkdir()
    work.mkdir()
    K.write_late_fixtures(str(refs), ftn)
    monkeypatch.chdir(work)                                               # `-o out.exr` of the lines would land here
    assert len(rec["late"]) == 9
    _same(K.late_answers(str(refs)), rec["late"])
    assert not list(work.iterdir())


def test_path_rules(rec):
    from fountain_amd._cli import beside
    assert [beside(n, "_x.exr") for n in K.PATH_NAMES] == ["out_x.exr", "a/out_x.exr", "out_x.exr", "out.exr.tmp_x.exr"]
    assert K.path_results() == rec["paths"]
    # lightpass_paths cuts at the last ".exr" wherever it stands, every other function only one at the end: the difference is kept
    assert rec["paths"]["out.exr.tmp"]["lightpass_paths"]["light"] == "out_light_point.exr"
    assert rec["paths"]["out.exr.tmp"]["ao_paths"]["ao"] == "out.exr.tmp_ao.exr" and rec["paths"]["out"]["lightpass_paths"] == "ValueError"


PURE = """
import json, sys
sys.path[:0] = %r
import _render_cli_cases as K
from fountain_amd import render
had = "torch" in sys.modules
out = [render.refusal(render.parser().parse_args([K.CORNELL, "-o", "out.exr"] + a)) for a in json.loads(sys.argv[1])]
print(json.dumps([out, had, "torch" in sys.modules]))
"""


def test_refusal_is_pure(rec):
    """refusal(opts) gives main's message without main: in a fresh interpreter, for 20 recorded lines (refused ones and ones that go
    on), and torch is not loaded by it"""
    lines = [a for a in K.singles_and_pairs() if isinstance(rec["lines"][K.key(a)], list)][::9][:16] + [["--gbuffer"], ["--png", "--bloom"], ["--gpus", "2"], ["--variance", "--adaptive", "0.05"]]
    assert len(lines) == 20
    p = subprocess.run([sys.executable, "-c", PURE % [ROOT, os.path.join(ROOT, "tests")], json.dumps(lines)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    got, had, has = json.loads(p.stdout)
    assert not had and not has
    want = [rec["lines"][K.key(a)] for a in lines]
    assert got == [w[1][len("error: "):-1] if isinstance(w, list) else None for w in want]
    assert len({g for g in got if g}) >= 8


@pytest.mark.gpu
def test_three_renders_write_what_they_wrote(gpu, tmp_path):
    """The files of an adaptive, a filtered and an everything-at-once render, their bytes, the metrics line and the order of the stderr
    lines equal the recording of the same three runs before render.main was split up."""
    want = json.load(open(K.OUTPUTS))
    got = K.render_outputs(tmp_path)
    assert sorted(got["files"]) == sorted(want["files"])
    assert got["stderr"] == want["stderr"]
    assert got["metrics"] == want["metrics"]
    assert got["files"] == want["files"]

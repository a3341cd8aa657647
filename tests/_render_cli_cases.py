"""The command lines of tests/test_render_cli.py and the recorder of what fountain_amd.render answers to them.

`python tests/_render_cli_cases.py --record` writes tests/golden/render_cli_refusals.json: per line the exit code and stderr of
render.main where it refuses before it loads the library or starts ranks, and "library" / "ranks" where it goes on (both are replaced by
functions that raise, so nothing renders and no rank starts).  `--record-outputs` (on a GPU) writes tests/golden/render_cli_outputs.json:
what three renders write.  Both are recorded on the commit whose behaviour is to be kept; this file uses nothing of the package but
render.main, launch.spawn_ranks, default_backend and write_exr."""
import contextlib
import hashlib
import io
import itertools
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CORNELL = os.path.join(GOLDEN, "cornell.pbrt")
FURNACE = os.path.join(GOLDEN, "furnace_empty.pbrt")                  # 16 x 16
REFUSALS = os.path.join(GOLDEN, "render_cli_refusals.json")
OUTPUTS = os.path.join(GOLDEN, "render_cli_outputs.json")
MISSING = "no_such_reference.exr"

GROUPS = (["--gbuffer"], ["--idmatte", "material"], ["--ao"], ["--light-groups"], ["--denoise"], ["--variance"], ["--denoise-guided"], ["--adaptive", "0.05"],
          ["--pixel-filter", "gaussian"], ["--png"], ["--exact-stream"], ["--gpus", "2"], ["--bloom"], ["--compare-to", MISSING], ["--min-samples", "4"],
          ["--ao-radius", "1"], ["--filter-width", "2"], ["--ssim"], ["--exposure", "1"], ["--bloom-levels", "3"])
GPUS2, GPUS1 = ["--gpus", "2"], ["--gpus", "1"]
WORLD = {"WORLD_SIZE": "3", "RANK": "0"}

BLOOM_SUBS = (["--bloom-levels", "3"], ["--bloom-scatter", "0.5"], ["--bloom-threshold", "1"], ["--bloom-knee", "0.5"], ["--bloom-karis"])
BLOOM_BAD = (["--bloom-levels", "13"], ["--bloom-levels", "-1"], ["--bloom-scatter", "1.5"], ["--bloom-scatter", "nan"], ["--bloom-threshold", "-1"],
             ["--bloom-threshold", "inf"], ["--bloom-knee", "2"], ["--bloom-knee", "-0.5"])
BAD_VALUES = ([["--ao", "0"], ["--ao", "65"], ["--ao", "--ao-radius", "0"], ["--ao-radius", "0"], ["--adaptive", "-1"], ["--adaptive", "inf"],
               ["--idmatte", "material,material"], ["--idmatte", "nope"], ["--pixel-filter", "gaussian", "--filter-width", "1", "2", "3"], ["--filter-width", "1", "2", "3"],
               ["--gamma", "2"], ["--png", "--gamma", "2"], ["--png", "--transfer", "srgb", "--gamma", "2"],
               ["--gpus", "0"], ["--gpus", "-3"], ["--gpus", "0", "--png"], ["--gpus", "0", "--gbuffer"]]    # started plainly, that is one rank: not 0 of them
              + [["--png"] + s for s in BLOOM_SUBS] + [["--bloom"], ["--bloom", "0.1", "--bloom-karis"], ["--png", "--bloom", "--gpus", "2"]]
              + [["--png", "--bloom", v] for v in ("1.5", "-0.5", "nan")] + [["--png", "--bloom"] + b for b in BLOOM_BAD])


def key(args):
    return " ".join(args)


def combos(n):
    return [sum(c, []) for c in itertools.combinations(GROUPS, n)]


def singles_and_pairs():
    return combos(1) + combos(2)


def with_gpus_1():
    """the singles and pairs that hold --gpus 2, with --gpus 1 in its place"""
    return [sum((GPUS1 if g == GPUS2 else g for g in c), []) for n in (1, 2) for c in itertools.combinations(GROUPS, n) if GPUS2 in c]


class GoesOn(Exception):
    """raised in place of loading the library ("library") or starting ranks ("ranks")"""


@contextlib.contextmanager
def stubbed():
    from fountain_amd import launch, render

    def stop(where):
        def raiser(*a, **k):
            raise GoesOn(where)
        return raiser
    saved = render.default_backend, launch.spawn_ranks
    render.default_backend, launch.spawn_ranks = stop("library"), stop("ranks")
    try:
        yield
    finally:
        render.default_backend, launch.spawn_ranks = saved


def answer(args, scene=CORNELL, names=()):
    """What render.main answers to `scene -o out.exr args`: [exit code, stderr], or "library" / "ranks" where a stub of stubbed() was
    reached.  `names` are (path, word) pairs replaced in stderr, so that a recording does not depend on where its files lay."""
    from fountain_amd import render
    err = io.StringIO()
    with contextlib.redirect_stderr(err):
        try:
            code = render.main([scene, "-o", "out.exr"] + list(args))
        except GoesOn as e:
            return str(e)
        except SystemExit as e:
            code = e.code
    text = err.getvalue()
    for path, word in tuple(names) + ((ROOT, "<root>"),):
        text = text.replace(path, word)
    return [code, text]


def answers(lines, env=None):
    saved = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        with stubbed():
            return {key(a): answer(a) for a in lines}
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def triple_messages(rec, groups):
    """the messages recorded for the singles and pairs of a triple of groups"""
    subs = [sum(c, []) for n in (1, 2) for c in itertools.combinations(groups, n)]
    return {rec["lines"][key(s)][1] for s in subs if isinstance(rec["lines"][key(s)], list)}


# ------------------------------------------------------------------ refusals that need the parsed scene
PLAIN_NAME = "plain.pbrt"


def write_late_fixtures(refs, be):
    """The files the scene-dependent lines read, written into the directory `refs`: references of other sizes than the films and a
    scene without a PixelFilter statement."""
    import numpy as np
    from fountain_amd.api import write_exr
    write_exr(os.path.join(refs, "wide.exr"), np.zeros((64, 48, 3), np.float32), be)
    write_exr(os.path.join(refs, "small.exr"), np.zeros((8, 8, 3), np.float32), be)
    with open(os.path.join(refs, "junk.exr"), "wb") as f:
        f.write(b"not an image")
    text = open(CORNELL).read()
    assert 'PixelFilter "box"\n' in text
    with open(os.path.join(refs, PLAIN_NAME), "w") as f:
        f.write(text.replace('PixelFilter "box"\n', ""))


def late_lines(refs):
    """(name, scene, args) of the lines that are refused after the scene file is parsed and before a scene is created"""
    r = lambda n: os.path.join(str(refs), n)
    return (("compare-to another size", CORNELL, ["--compare-to", r("wide.exr")]),
            ("compare-to another size with ssim", CORNELL, ["--compare-to", r("wide.exr"), "--ssim"]),
            ("compare-to unreadable", CORNELL, ["--compare-to", r("junk.exr")]),
            ("compare-to ssim below 11 x 11", FURNACE, ["--compare-to", r("small.exr"), "--ssim"]),
            ("denoise-guided at 1 spp", CORNELL, ["--denoise-guided", "--samples", "1"]),
            ("min-samples above samples", CORNELL, ["--samples", "4", "--adaptive", "0.05", "--min-samples", "8"]),
            ("min-samples default above samples", CORNELL, ["--samples", "1", "--adaptive", "0.05"]),
            ("min-samples below 2", CORNELL, ["--samples", "8", "--adaptive", "0.05", "--min-samples", "1"]),
            ("pixel-filter scene without a statement", r(PLAIN_NAME), ["--pixel-filter", "scene"]))


def late_answers(refs):
    """{name: [exit code, stderr]} of late_lines with the real library; the caller has replaced PbrtScene.create_scene if it wants to."""
    return {name: answer(args, scene, names=((str(refs), "<refs>"),)) for name, scene, args in late_lines(refs)}


# ------------------------------------------------------------------ the path rules
PATH_NAMES = ("out.exr", "a/out.exr", "out", "out.exr.tmp")


def path_results():
    """What every *_path(s) function of render and temporal gives for PATH_NAMES (tuples as lists, as JSON holds them)."""
    from fountain_amd import render, temporal
    out = {}
    for name in PATH_NAMES:
        r = {f: getattr(render, f)(name) for f in ("gbuffer_paths", "denoised_path", "denoised_guided_path", "variance_path", "bloom_path", "spp_path", "idmatte_path",
                                                  "ao_paths", "png_path")}
        # lightpass_paths cuts at the LAST ".exr" wherever it stands (rindex), the others only an ".exr" at the end: out.exr.tmp differs,
        # and a name without ".exr" is an error there
        try:
            r["lightpass_paths"] = render.lightpass_paths(name, "point")
        except ValueError:
            r["lightpass_paths"] = "ValueError"
        r.update({f: getattr(temporal, f)(name, 3) for f in ("motion_path", "blurred_path", "frame_paths")})
        out[name] = json.loads(json.dumps(r))
    return out


# ------------------------------------------------------------------ three renders and what they write (GPU)
def head(line):
    """a stderr line up to its first ':'; "Completed rendering in 0.069 s (...)" has none and is cut in front of its first digit"""
    return line.split(":", 1)[0] if ":" in line else re.split(r"\d", line, maxsplit=1)[0]


def render_outputs(tmp):
    """Three runs of render.main on cornell.pbrt with 4 samples into the directory `tmp`.  Returns {"files": {name: sha256}, "metrics":
    the metrics line of run 3, "stderr": per run the head() of each stderr line (the lines carry timings)}."""
    from fountain_amd import render
    first = os.path.join(str(tmp), "one.exr")
    runs = ((first, ["--adaptive", "0.05", "--min-samples", "2", "--variance"]),
            (os.path.join(str(tmp), "two.exr"), ["--pixel-filter", "gaussian", "--png", "--auto-exposure"]),
            (os.path.join(str(tmp), "three.exr"), ["--gbuffer", "--idmatte", "material,shape", "--ao", "2", "--light-groups", "kind", "--denoise", "--denoise-guided",
                                                   "--variance", "--png", "--bloom", "--compare-to", first, "--ssim"]))
    heads, metrics = [], []
    for out, extra in runs:
        o, e = io.StringIO(), io.StringIO()
        with contextlib.redirect_stdout(o), contextlib.redirect_stderr(e):
            code = render.main([CORNELL, "-o", out, "--samples", "4"] + extra)
        assert code == 0, (extra, e.getvalue())
        heads.append([head(line) for line in e.getvalue().splitlines()])
        metrics += [line for line in o.getvalue().splitlines() if line.startswith("metrics:")]
    files = {n: hashlib.sha256(open(os.path.join(str(tmp), n), "rb").read()).hexdigest() for n in sorted(os.listdir(str(tmp)))}
    assert len(metrics) == 1, metrics
    return {"files": files, "metrics": metrics[0], "stderr": heads}


def record():
    import tempfile
    from fountain_amd import default_backend
    rec = {"lines": answers(singles_and_pairs()), "triples": {k: (v if isinstance(v, str) else v[0]) for k, v in answers(combos(3)).items()},
           "gpus_1": answers(with_gpus_1()), "launcher": answers([[]] + combos(1), env=WORLD), "bad_values": answers(BAD_VALUES)}
    with tempfile.TemporaryDirectory() as refs:
        write_late_fixtures(refs, default_backend())
        rec["late"] = late_answers(refs)
    rec["paths"] = path_results()
    json.dump(rec, open(REFUSALS, "w"), indent=0, sort_keys=True)
    kinds = [("refused" if isinstance(v, list) else v) for v in rec["lines"].values()]
    print({k: kinds.count(k) for k in sorted(set(kinds))}, "triples refused:", sum(v == 2 for v in rec["triples"].values()), "of", len(rec["triples"]))


def record_outputs(path):
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        json.dump(render_outputs(tmp), open(path, "w"), indent=0, sort_keys=True)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    if sys.argv[1:2] == ["--record"]:
        record()
    elif sys.argv[1:2] == ["--record-outputs"]:
        record_outputs(sys.argv[2] if len(sys.argv) > 2 else OUTPUTS)
    else:
        sys.exit("usage: _render_cli_cases.py --record | --record-outputs [FILE]")

"""Corrupt PBRT, PLY and OpenEXR files (tests/_corrupt_files.py) against the library's readers: ftn_pbrt_load, ftn_ply_load, ftn_exr_read.

CPU only.  Each (reader, seed) family is walked by one fresh child process that loads the library with ctypes; the child notes every case
in a progress file before the call, so a crash or a hang fails the family's test by the name of the case and does not end the pytest
run.  After a crash the walk is taken up behind the case that crashed, so that every crashing case of a family is named.  The contract
a case is held to is in _corrupt_files.py's docstring.  The sanitizer build of the same corpus is tools/reader_check.cpp, built and run
here as a program of its own (nothing is preloaded)."""
import json
import os
import shutil
import subprocess
import sys

import pytest

import _corrupt_files as CF

HANG_LIMIT = 120           # seconds for a whole child: a hang detector, not a timing
MAX_CRASHES = 12           # crashes named per family before the walk is given up
ROOT = os.path.dirname(CF.HERE)

_reports = {}


def _last_case(progress):
    try:
        with open(progress, "rb") as f:
            lines = f.read().decode(errors="replace").splitlines()
    except OSError:
        lines = []
    return len(lines), (lines[-1] if lines else "(before the first case)")


def walk_family(name, tmp):
    """-> dict(failures=[(case, what)], n_cases, n_random, n_random_ok), from as many child processes as there were crashes, plus one."""
    if name in _reports:
        return _reports[name]
    total = dict(failures=[], n_cases=0, n_random=0, n_random_ok=0)
    start = 0
    for attempt in range(MAX_CRASHES + 1):
        scratch = os.path.join(tmp, "%s-%d" % (name, attempt))
        os.makedirs(scratch)
        progress, report = os.path.join(scratch, "progress.txt"), os.path.join(scratch, "report.json")
        cmd = [sys.executable, os.path.join(CF.HERE, "_corrupt_files.py"), "--walk", name, "--lib", CF.default_library(), "--scratch", scratch,
               "--progress", progress, "--report", report, "--start", str(start)]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=HANG_LIMIT)
            hung = False
        except subprocess.TimeoutExpired:
            hung = True
        if os.path.exists(report):
            r = json.load(open(report))
            total["failures"] += [tuple(f) for f in r["failures"]]
            for k in ("n_cases", "n_random", "n_random_ok"):
                total[k] += r[k]
            if r["done"] and not hung and p.returncode == 0:
                break
        n_lines, last = _last_case(progress)
        if hung:
            total["failures"].append((last, "did not return within %d s (the walk of this family ends here)" % HANG_LIMIT))
            break
        tail = p.stdout.decode(errors="replace").strip().splitlines()[-3:]
        total["failures"].append((last, "the child process ended with status %d: %s" % (p.returncode, " | ".join(tail))))
        if n_lines < 2 or attempt == MAX_CRASHES:        # it never reached a case, or enough has been named
            break
        start += n_lines - 1                             # the first line is the untouched seed; take the walk up behind the case that crashed
        shutil.rmtree(scratch, ignore_errors=True)
    _reports[name] = total
    return total


@pytest.fixture(scope="module")
def walk_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("corrupt_files"))


@pytest.mark.parametrize("name", CF.family_names())
def test_corrupt_files_are_refused_or_read_consistently(ftn, walk_dir, name):
    r = walk_family(name, walk_dir)
    share = r["n_random_ok"] / max(1, r["n_random"])
    print("%s: %d cases, %d of %d random single-byte changes accepted (%.1f %%)" % (name, r["n_cases"], r["n_random_ok"], r["n_random"], 100 * share))
    assert not r["failures"], "%s: %d cases fail:\n%s" % (name, len(r["failures"]), "\n".join("  [%s] %s" % f for f in r["failures"]))
    assert r["n_random"] == CF.N_RANDOM and r["n_cases"] > CF.N_RANDOM
    # the family's own ceiling: the bytes the format leaves free (CF.free_share) may all be accepted, and of the others the 40 % the
    # bound below allows overall -- so that one reader losing its checks is noticed though the other families dilute it
    reader, seed, _ = CF.family(name, CF.writer_of(CF.load_library(CF.default_library()), walk_dir))
    free = CF.free_share(name, seed)
    ceiling = free + 0.40 * (1.0 - free)
    print("%s: %.1f %% of the seed's bytes are free by the format, ceiling %.1f %%" % (name, 100 * free, 100 * ceiling))
    assert share <= ceiling, "%s: %.1f %% of the random single-byte changes are accepted, ceiling %.1f %%" % (name, 100 * share, 100 * ceiling)


def test_most_random_single_byte_changes_are_refused(ftn, walk_dir):
    """At most 40 % of the random single-byte cases may end in FTN_OK.  The bytes that are legitimately free are the pixel and vertex
    payload of the uncompressed seeds, the numbers, comments and white space of the scene text, and the attributes and header fields
    the readers have no use for ("File readers"); the share is taken over the random cases of all families together, since
    one seed alone -- 5 x 17 FLOAT pixels without compression are 1020 free bytes of 1578 -- says how large its payload is, not how
    much the reader checks; each family has a ceiling of its own in the test above."""
    n = ok = 0
    for name in CF.family_names():
        r = walk_family(name, walk_dir)
        print("%-34s %4d of %4d accepted (%.1f %%)" % (name, r["n_random_ok"], r["n_random"], 100 * r["n_random_ok"] / max(1, r["n_random"])))
        n += r["n_random"]; ok += r["n_random_ok"]
    print("all families: %d of %d accepted (%.1f %%)" % (ok, n, 100 * ok / max(1, n)))
    assert n == CF.N_RANDOM * len(CF.family_names())
    assert ok <= 0.40 * n, "%d of %d random single-byte changes were accepted" % (ok, n)


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc to build tools/reader_check.cpp")
def test_reader_check_under_address_and_undefined_behaviour_sanitizers(ftn, tmp_path):
    """tools/reader_check.cpp: the readers' host code linked with ASan + UBSan into a program of its own, run over the whole corpus
    (sizing call, then the filling call into exactly-sized heap buffers; accepted scenes go on to the host-only ftn_bvh_build)."""
    import time
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    corpus = str(tmp_path / "corpus")
    t0 = time.time()
    n = CF.write_corpus(corpus, CF.default_library())
    t1 = time.time()
    exe = str(tmp_path / "reader_check")
    csrc = os.path.join(ROOT, "fountain_amd", "csrc")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    cmd = [hipcc, "-std=c++17", "-O1", "-g", "-x", "hip", "--cuda-host-only"] + san + \
          [os.path.join(ROOT, "tools", "reader_check.cpp")] + [os.path.join(csrc, f) for f in ("ftn_pbrt.cpp", "ftn_imageio.cpp", "ftn_geometry_host.cpp", "ftn_scene_host.cpp", "ftn_bvh_host.cpp")] + \
          ["-I" + csrc, "-fsanitize=address,undefined", "-lz", "-o", exe]
    b = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert b.returncode == 0, b.stdout.decode(errors="replace")[-4000:]
    t2 = time.time()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:allocator_may_return_null=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, corpus, os.path.join(corpus, "manifest.txt")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600, env=env)
    out = r.stdout.decode(errors="replace")
    print("corpus of %d files written in %.1f s, reader_check built in %.1f s and run in %.1f s" % (n, t1 - t0, t2 - t1, time.time() - t2))
    assert r.returncode == 0 and "reader_check: ok" in out, out[-4000:]
    assert "%d files" % n in out, out[-400:]

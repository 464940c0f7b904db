"""The GMRF_* environment variables the library reads are exactly those tools/README.md lists.

A form selected by a user-set variable is a form no test, benchmark or caller runs; the ones that remain are public
(include/gmrf_hip.h), set by a test, or a field of a kernel waiting for that kernel's measurement.  A new read has to
be added to the list -- with its reason -- before this passes."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "diffeqgmrfs.jl_amd")

# getenv("GMRF_X") and the helper env_int("GMRF_X", default) of host_util.hpp; os.environ.get("GMRF_X") / os.environ["GMRF_X"]
NATIVE_READ = re.compile(r'\b(?:getenv|env_int)\(\s*"(GMRF_[A-Z0-9_]+)"')
PYTHON_READ = re.compile(r'\benviron(?:\.get\(|\[)\s*"(GMRF_[A-Z0-9_]+)"')


def names_read():
    native = sorted(glob.glob(os.path.join(PKG, "csrc", "*.hip")) + glob.glob(os.path.join(PKG, "csrc", "*.hpp")))
    assert native, "no native sources found"
    found, getenv_calls, getenv_named = set(), 0, 0
    for path in native:
        with open(path) as fh:
            text = fh.read()
        found.update(NATIVE_READ.findall(text))
        getenv_calls += len(re.findall(r"\bgetenv\(", text))
        getenv_named += len(re.findall(r'\bgetenv\(\s*"GMRF_', text))
    # every getenv names its variable in place, but for the one inside env_int: no name is put together out of sight of the scan
    assert getenv_calls == getenv_named + 1, (getenv_calls, getenv_named)
    with open(os.path.join(PKG, "_cabi.py")) as fh:
        text = fh.read()
    found.update(PYTHON_READ.findall(text))
    assert len(re.findall(r"\benviron\b", text)) == len(PYTHON_READ.findall(text))
    return found


def names_listed():
    with open(os.path.join(ROOT, "tools", "README.md")) as fh:
        paragraphs = fh.read().split("\n\n")
    env, = [p for p in paragraphs if p.lstrip().startswith("Environment variables read by the library")]
    return set(re.findall(r"`(GMRF_[A-Z0-9_]+)`", env))


def test_environment_reads_match_the_documented_list():
    read, listed = names_read(), names_listed()
    assert read == listed, {"read but not listed": sorted(read - listed), "listed but not read": sorted(listed - read)}
    assert {"GMRF_RCCL_PATH", "GMRF_VAR_STAGE_MB", "GMRF_HIP_LIBRARY"} <= read      # the public ones (include/gmrf_hip.h)

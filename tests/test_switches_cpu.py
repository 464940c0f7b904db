"""The route switches have one set of names: the GMRF_SW_* enumerators of include/gmrf_hip.h, the package's `Switch` members and
the table below say the same (name, bit) pairs -- the numbers are ABI (recorded profiles, tools/ab_sweep.sh and
`bench.py --eager-flags` carry them) -- and no test or tool passes set_eager a bare number any more."""
import glob
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CC = os.environ.get("CC", "cc")

BITS = {"EAGER": 0, "BATCH_ROUTES": 1, "SWEEP_NO_GEMM": 2, "DENSE_COUPLING": 3, "FORK_GRAPH": 4, "NO_STAIRCASE": 5,
        "DOUBLING_INVERSE": 7, "NO_LOOKAHEAD": 8, "NO_XSPLIT": 12, "NO_PERSIST": 13, "NO_PERSIST_PANELS": 15,
        "NO_SWEEP_PERSIST": 16, "NO_SCATTER_FOLD": 17, "TWO_CALL_POSTERIOR": 18, "NO_FACTOR_FWD": 19, "NO_GROUPED_GEMM": 20,
        "NO_ENVELOPE": 21}

# set_eager( followed by a number that is not 0: only these files may, and why
PASSTHROUGH = {"tools/stream_sweep.py"}      # forwards GMRF_EAGER_FLAGS, a number by design
LITERAL = re.compile(r"set_eager\(\s*(?:int\()?\s*(\d+|True|False)\b")


def header_enumerators(tmp_path):
    with open(os.path.join(ROOT, "include", "gmrf_hip.h")) as fh:
        names = sorted(set(re.findall(r"\bGMRF_SW_[A-Z0-9_]+\b", fh.read())))
    src = tmp_path / "switches.c"
    src.write_text('#include <stdio.h>\n#include "gmrf_hip.h"\nint main(void) {\n'
                   + "".join(f'    printf("{n} %ld\\n", (long){n});\n' for n in names) + "    return 0;\n}\n")
    exe = str(tmp_path / "switches")
    build = subprocess.run([CC, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)],
                           capture_output=True, text=True, timeout=120)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    return {(line.split()[0][len("GMRF_SW_"):], int(line.split()[1])) for line in run.stdout.splitlines()}


def test_header_package_and_table_name_the_same_bits(tmp_path):
    import __graft_entry__ as g
    pkg = g.load_package()
    header = header_enumerators(tmp_path)
    assert header == {(m.name, m.value) for m in pkg.Switch}
    assert header == {(name, 1 << bit) for name, bit in BITS.items()}
    assert len(BITS) == 17


def test_no_caller_passes_set_eager_a_bare_number():
    paths = sorted(glob.glob(os.path.join(ROOT, "tests", "*.py")) + glob.glob(os.path.join(ROOT, "tools", "*.py")))
    assert len(paths) > 40
    found = []
    for path in paths:
        name = os.path.relpath(path, ROOT)
        if name in PASSTHROUGH or name == os.path.relpath(os.path.abspath(__file__), ROOT):
            continue
        with open(path) as fh:
            for no, line in enumerate(fh, 1):
                found += [(name, no, m.group(1)) for m in LITERAL.finditer(line) if m.group(1) not in ("0", "1", "True", "False")]
    assert not found, found

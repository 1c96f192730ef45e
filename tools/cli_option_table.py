"""The option table of every command-line script: for each main_*.py, the parser's description and, per option, its
strings, dest, nargs, type, default, choices, required and help.  tests/golden/cli_options.json is this table as recorded
before the scripts were rebuilt on audioeditingcode_amd/cli.py; tests/test_cli_cpu.py regenerates and compares it.

python tools/cli_option_table.py [out.json]          (stdout without a path)
"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SCRIPTS = ["main_run", "main_run_variants", "main_run_batch", "main_run_sa_variants", "main_run_sa_batch", "main_run_grid",
           "main_run_segments", "main_run_sdedit", "main_pc_extract_inv", "main_pc_apply_drift", "main_pc_apply_drift_grid"]


class _Captured(Exception):
    pass


def parser_of(script):
    """The ArgumentParser the script builds, caught at its parse_args call: before any validation, so no argv is needed."""
    mod = importlib.import_module(f"audioeditingcode_amd.{script}")
    real = argparse.ArgumentParser.parse_args

    def capture(self, *a, **k):
        raise _Captured(self)
    argparse.ArgumentParser.parse_args = capture
    try:
        if hasattr(mod, "parse_args"):
            mod.parse_args([])
        else:
            mod.build_parser().parse_args([])
    except _Captured as c:
        return c.args[0]
    finally:
        argparse.ArgumentParser.parse_args = real
    raise RuntimeError(f"{script}: no ArgumentParser.parse_args call was reached")


def table():
    out = {}
    for script in SCRIPTS:
        p = parser_of(script)
        out[script] = dict(description=p.description, options=[
            dict(option_strings=list(a.option_strings), dest=a.dest, nargs=a.nargs,
                 type=None if a.type is None else a.type.__name__, default=a.default,
                 choices=None if a.choices is None else list(a.choices), required=a.required, help=a.help)
            for a in p._actions])
    return json.loads(json.dumps(out))


if __name__ == "__main__":
    text = json.dumps(table(), indent=1) + "\n"
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)

"""Extract the argparse flags of the reference CLIs (read as text with `ast`, nothing imported)
into tests/golden/cli_flags.json: {"<folder>/<script>": {flag: {type, default, required, choices,
action}}}.  tests/test_cli_cpu.py checks vclip_amd.apps' parsers against it.

    python tools/make_cli_flags.py                                        the four folders -> cli_flags.json
    python tools/make_cli_flags.py resnet50-2d-lstm cli_flags_lstm.json   one folder -> its own file
                                                                          (tests/test_lstm_cli_cpu.py)
"""
import ast
import json
import os
import sys

REF = os.environ.get("VCLIP_REFERENCE", "/root/reference")
GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
OUT = os.path.join(GOLDEN, "cli_flags.json")
FOLDERS = ("vivit_transformer", "timesformer", "videoswintransformer", "resnet50-3d-video")
SCRIPTS = [f"{d}/{s}.py" for d in FOLDERS for s in ("main", "inference")]


def lit(node):
    try:
        return ast.literal_eval(node)
    except Exception:
        return ast.unparse(node)


def flags(path):
    out = {}
    for n in ast.walk(ast.parse(open(path).read())):
        if isinstance(n, ast.Call) and getattr(n.func, "attr", None) == "add_argument":
            name = lit(n.args[0])
            kw = {k.arg: lit(k.value) for k in n.keywords if k.arg in ("type", "default", "required", "choices", "action")}
            out[name] = kw
    return out


if __name__ == "__main__":
    scripts, out = SCRIPTS, OUT
    if len(sys.argv) == 3:
        scripts, out = [f"{sys.argv[1]}/{s}.py" for s in ("main", "inference")], os.path.join(GOLDEN, sys.argv[2])
    elif len(sys.argv) != 1:
        sys.exit(__doc__)
    res = {s: flags(os.path.join(REF, s)) for s in scripts}
    json.dump(res, open(out, "w"), indent=1, sort_keys=True)
    print(out, sum(len(v) for v in res.values()), "flags", file=sys.stderr)

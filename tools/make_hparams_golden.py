"""Generate tests/golden/hparams_chains.json: for each yaml chain tests/test_host_logic.py checks, the files of the chain (as
parsed yaml, by their path relative to the reference root) and what the REFERENCE's own utils/commons/hparams.py resolves the
chain to (run in a subprocess), given a checkout of the reference:

    PYTHONDONTWRITEBYTECODE=1 python tools/make_hparams_golden.py <reference root>

The fixture holds parser inputs + expected outputs only (no reference source).
"""
import json
import os
import subprocess
import sys

import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)

from conan_amd.utils.commons import hparams as hpm  # noqa: E402

CONFIGS = ("egs/conan_emformer.yaml", "egs/hifi_16k320_shuffle.yaml")
OUT = os.path.join(REPO, "tests", "golden", "hparams_chains.json")


def reference_resolve(root, cfg):
    code = ("import json,sys; sys.dont_write_bytecode=True\n"
            "from utils.commons.hparams import set_hparams\n"
            f"hp = set_hparams(config={cfg!r}, exp_name='', print_hparams=False, global_hparams=False)\n"
            "print('JSON' + json.dumps(hp, sort_keys=True, default=str))\n")
    env = dict(os.environ, PYTHONPATH=root, PYTHONDONTWRITEBYTECODE="1")
    out = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True, timeout=120, check=True)
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("JSON")][-1][4:])


def chain_files(root, cfg):
    """path relative to root -> parsed yaml, for every file the chain of `cfg` reads."""
    chain = []
    cwd = os.getcwd()
    try:
        os.chdir(root)
        hpm._load_chain(cfg, set(), chain)
        files = {}
        for p in chain:
            with open(p) as f:
                d = yaml.safe_load(f) or {}
            assert yaml.safe_load(yaml.safe_dump(d)) == d, p      # the test writes the files back with safe_dump
            files[p] = d
        return files
    finally:
        os.chdir(cwd)


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    root = sys.argv[1]
    out = {cfg: {"files": chain_files(root, cfg), "resolved": reference_resolve(root, cfg)} for cfg in CONFIGS}
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()

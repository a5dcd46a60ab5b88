"""The configs the reference ships, as data (TEST INFRASTRUCTURE; needs a checkout of the reference).

tests/test_config.py::test_shipped_golf_configs_instantiate builds every GOLF / DDSP / NHV / WORLD config of the reference
on this package's classes.  This script parses each of those YAML files and keeps only what golf_amd.config.build_model
reads -- the ``model`` section (of an ISMIR'23 Lightning module: its ``decoder``), or a bare ``decoder`` file's
``decoder`` -- plus the nodes its ``${a.b.c}`` references point to; trainer, data, logger and callback sections are dropped.
The kept values are re-serialised by yaml.safe_dump (no comments, no layout of the original files), so that the test runs
from a checkout of this repository alone.  References are kept as written: resolving them is part of what the test exercises.

    python oracle/make_config_fixtures.py REFERENCE_CHECKOUT     ->  tests/golden/g28_shipped_configs.npz
"""
import os
import re
import sys

import numpy as np
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from golf_amd.config import _interpolate  # noqa: E402

FILES = ["cfg/ae/decoder/golf.yaml", "cfg/ae/decoder/golf-precise.yaml", "cfg/ae/decoder/golf-v1.yaml",
         "cfg/ae/decoder/ddsp.yaml", "ckpts/interspeech24/golf-ss/config.yaml",
         "ckpts/interspeech24/golf-ff/config.yaml", "ckpts/interspeech24/golf-v1/config.yaml",
         "ckpts/interspeech24/ddsp/config.yaml", "cfg/ae/decoder/nhv.yaml",
         "ckpts/interspeech24/nhv/config.yaml", "cfg/ae/decoder/world.yaml",
         "ckpts/interspeech24/world/config.yaml"] + [f"ckpts/ismir23/{m}_{v}/config.yaml"
                                                    for m in ("glottal_d", "ddsp", "pulse", "sawsing")
                                                    for v in ("f1", "m1")]
REF = re.compile(r"^\$\{([\w.]+)\}$")   # the reference syntax golf_amd.config._interpolate resolves


def used_path(tree):
    """The keys of the node build_model instantiates (same order of tests as golf_amd.config.build_model)."""
    if "model" in tree:
        model = tree["model"]
        return ["model", "decoder"] if "class_path" not in model and "decoder" in model else ["model"]
    return ["decoder"] if "decoder" in tree else []


def get(tree, keys):
    for k in keys:
        tree = tree[int(k)] if isinstance(tree, list) else tree[k]
    return tree


def put(dst, src, keys):
    """Copy the node at ``keys`` of ``src`` into ``dst``, creating the dicts on the way."""
    for k in keys[:-1]:
        src = src[k]
        dst = dst.setdefault(k, {})
    dst[keys[-1]] = src[keys[-1]]


def refs(node):
    if isinstance(node, str):
        m = REF.match(node)
        return [m.group(1).split(".")] if m else []
    if isinstance(node, dict):
        return [r for v in node.values() for r in refs(v)]
    if isinstance(node, list):
        return [r for v in node for r in refs(v)]
    return []


def keep_used(tree):
    path = used_path(tree)
    kept = {}
    if path:
        put(kept, tree, path)
    else:
        kept.update(tree)
    while True:   # the nodes the references point to (which may hold references of their own)
        missing = []
        for r in refs(kept):
            try:
                get(kept, r)
            except (KeyError, IndexError, TypeError):
                missing.append(r)
        if not missing:
            break
        for r in missing:
            put(kept, tree, r)   # (put walks dicts only: a reference into a list fails here, loudly)
    # what build_model sees is unchanged
    assert get(_interpolate(kept), path) == get(_interpolate(tree), path)
    return kept


def main(ref):
    texts = []
    for rel in FILES:
        with open(os.path.join(ref, rel)) as f:
            tree = keep_used(yaml.safe_load(f))
        text = yaml.safe_dump(tree, sort_keys=False)
        assert yaml.safe_load(text) == tree, rel   # the stored text parses back to exactly the kept values
        texts.append(text)
    out = os.path.join(ROOT, "tests", "golden", "g28_shipped_configs.npz")
    np.savez_compressed(out, path=np.array(FILES), config=np.array(texts))
    print(out, len(FILES), "configs", os.path.getsize(out), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit("usage: make_config_fixtures.py REFERENCE_CHECKOUT")
    main(sys.argv[1])

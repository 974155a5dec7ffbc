#!/usr/bin/env python3
"""Writes tests/golden/reference_configs.json: the ``model:`` mapping and ``data.img_size`` of each of the reference's shipped configs
(``src/configs/*.yml``), read from a reference checkout.  Only these values are stored, so tests/test_cpu_dropin.py runs without one:

    python tests/golden/make_reference_configs.py <reference checkout>
"""
import glob
import json
import os
import re
import sys

import yaml

HERE = os.path.dirname(os.path.abspath(__file__))


def model_section(path):
    """(``model:`` mapping, ``data.img_size``) of a reference config.  Baseline_ProtoPNet.yml does not parse as a whole (a stray comma in
    its ``data:`` section, ``:68``), so the top-level ``model:`` block is cut out as text and parsed on its own."""
    text = open(path).read()
    m = re.search(r"^model:.*?\n(?=^\S)", text, flags=re.S | re.M)
    model_config = yaml.safe_load(m.group(0))["model"]
    img_size = int(re.search(r"^data:.*?^  img_size:\s*(\d+)", text, flags=re.S | re.M).group(1))
    return model_config, img_size


if __name__ == "__main__":
    REF = sys.argv[1]
    out = {}
    for path in sorted(glob.glob(os.path.join(REF, "src", "configs", "*.yml"))):
        model_config, img_size = model_section(path)
        out[os.path.basename(path)] = {"model": model_config, "img_size": img_size}
    assert out, f"no configs under {REF}/src/configs"
    with open(os.path.join(HERE, "reference_configs.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(f"wrote {len(out)} configs")

#!/usr/bin/env python3
"""Writes tests/golden/reference_criterion_configs.json: the ``train.criterion`` mapping and the top-level ``abstain_class`` of each of
the reference's four XProto configs (``src/configs/*.yml`` whose criterion has a ``ClusterRoiFeat`` entry), read from a reference
checkout.  As in make_reference_configs.py the block is cut out as text and parsed on its own, and only the values are stored, so
tests/test_cpu_proto_loss.py runs without a checkout:

    python tests/golden/make_reference_criterion_configs.py <reference checkout>
"""
import glob
import json
import os
import re
import sys

import yaml

HERE = os.path.dirname(os.path.abspath(__file__))


def criterion_section(path):
    """(``train.criterion`` mapping, ``abstain_class``) of a reference config: the block runs from its ``  criterion:`` line to the next
    key at the same or a lower indentation."""
    text = open(path).read()
    m = re.search(r"^  criterion:.*?\n(?=^ {0,2}\S)", text, flags=re.S | re.M)
    criterion = yaml.safe_load(m.group(0))["criterion"]
    a = re.search(r"^abstain_class:\s*(\w+)", text, flags=re.M)
    return criterion, bool(a) and a.group(1).lower() == "true"


if __name__ == "__main__":
    REF = sys.argv[1]
    out = {}
    for path in sorted(glob.glob(os.path.join(REF, "src", "configs", "*.yml"))):
        criterion, abstain = criterion_section(path)
        if "ClusterRoiFeat" in criterion:
            out[os.path.basename(path)] = {"criterion": criterion, "abstain_class": abstain}
    assert len(out) == 4, f"expected the four XProto configs under {REF}/src/configs, found {sorted(out)}"
    with open(os.path.join(HERE, "reference_criterion_configs.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(f"wrote {len(out)} configs")

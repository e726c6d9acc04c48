#!/usr/bin/env python3
"""Extract the reference's shipped code table, PosNoeudsVariable (Constants/50GPON-dc-original/Constants_SSE.h:29-3102),
into tests/golden/pos_noeuds_variable.npy (70400 VN indices, uint16) for tests/test_tables_and_abi.py.

Data only: the numbers of the initialiser are parsed (comments dropped) and stored; no reference source text is stored.
Run where the reference is available:  python tools/extract_pos_table.py <reference>/Constants/50GPON-dc-original/Constants_SSE.h
"""
import hashlib
import os
import re
import sys

import numpy as np

if len(sys.argv) != 2:
    raise SystemExit(__doc__)
text = open(sys.argv[1]).read()
i = text.index("{", text.index("_PosNoeudsVariable_"))
body = re.sub(r"/\*.*?\*/", "", text[i + 1:text.index("};", i)])
pos = np.array([int(x) for x in re.findall(r"\d+", body)], dtype=np.uint16)
assert pos.size == 70400, pos.size
out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "pos_noeuds_variable.npy")
np.save(out, pos)
print("entries", pos.size, "sha256 (<u2)", hashlib.sha256(pos.astype("<u2").tobytes()).hexdigest())

"""Writes tests/golden/store_v1: the store that pins format version 1 of mirx.store (tests/test_store_cpu.py).  Three rows of
dim 8 in two flushes, then id 1 deleted.  Run once per format version; a later version keeps reading this directory."""
import os
import shutil
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from mirx.store import Store  # noqa: E402

root = os.path.join(HERE, "store_v1")
shutil.rmtree(root, ignore_errors=True)
rows = (np.arange(24, dtype=np.float32).reshape(3, 8) - 7) / 4
col = Store(root).create("pinned", 8, "COSINE", ["id", "image_path", "label", "embedding"], "format pin")
col.append([0, 1], rows[:2], {"image_path": ["a.png", "b.png"], "label": [0, 1]})
col.flush()
col.append([2], rows[2:], {"image_path": ["c é.png"], "label": [None]})
col.delete([1])
col.flush()

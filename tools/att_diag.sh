#!/bin/bash
# phase attribution of k_attention_split from its diagnostic builds (make diag-src SRC=k_attention_split NAME=att_expM FLAGS=-DMIRX_ATT_EXP=M;
# bits: 1 no softmax arithmetic, 2 no tile staging, 4 no P V MFMAs, 8 no Q K MFMAs, 16 no barrier; results wrong, timing only;
# the bits act on both schemes, so the split-2 (fp16) and split-3 (bf16) lines are shown)
ROOT=$(cd "$(dirname "$0")/.." && pwd)
cd "$ROOT"
echo "shipped:"; python tools/bench_attention.py --iters 20 2>&1 | grep "split-[23]"
for m in "$@"; do echo "MIRX_ATT_EXP=$m:"; MIRX_LIB_PATH=$ROOT/exp/libatt_exp$m.so python tools/bench_attention.py --iters 20 2>&1 | grep "split-[23]"; done

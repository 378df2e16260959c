#!/bin/bash
# round 5 A/B on the GPU box: fused q/k/v epilogue on / off, GEMM tile-order group size (main-only bench lines, 20 steps each)
OUT=${1:?usage: r05_ab.sh <out_dir>}; mkdir -p $OUT
run() { tag=$1; shift; env "$@" timeout 300 python bench.py --full --main-only --steps 20 --no-cpu-baseline > $OUT/r05_ab_$tag.json 2> $OUT/r05_ab_$tag.err; python - <<PY
import json
try:
    d=json.load(open("$OUT/r05_ab_$tag.json")); r=d["roofline"]["per_step_ms"]
    print("$tag", "value", round(d["value"],2), "ms", round(d["ms_per_step"],2), "gemm", r.get("gemm_bt_p4<256,256>"), "qkv_post", r.get("qkv_post_vit"), r.get("qkv_post_llm"), "rms", r.get("rmsnorm"))
except Exception as e:
    print("$tag FAILED", e); print(open("$OUT/r05_ab_$tag.err").read()[-1500:])
PY
}
run fused_on  X=1
run fused_off FO1_QKV_FUSED=0
run ab_gm8 FO1_AB=1
run ab_gm4 FO1_AB=1 FO1_GEMM_GROUP_M=4
run ab_gm2 FO1_AB=1 FO1_GEMM_GROUP_M=2

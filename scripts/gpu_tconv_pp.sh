#!/bin/bash
# round 6: the pipelined persistent form of rw_tconv.hip (RW_TCONV_TY=2) against the specialised one (0) -- parity, then
# stand-alone times per layer
out=gpurun_out/${1:-r06e}; mkdir -p $out
timeout 900 python -m pytest tests/test_gpu_kernels.py -x -q -k "fused_transposed_conv_and_blur and pipelined" > $out/pytest_pp.log 2>&1; tail -3 $out/pytest_pp.log
for ty in 0 2; do
  RW_TCONV_TY=$ty RW_TCONV_ONLY=1 RW_LAYERS=layer13,layer15,layer17 timeout 300 python scripts/tconv_bench.py > $out/tconv_bench_ty$ty.jsonl 2>&1; echo "form $ty"; grep fused_ms $out/tconv_bench_ty$ty.jsonl
done

# developer sweep: evaluate()-pass latency vs batch with the GEMMs on large tiles (SE_AMD_GEMM_SMALL_M=0) or on the 128 x 128 kernel
# (SE_AMD_GEMM_SMALL_M=1000000), with / without the fused GEMM+LN kernel: where the small-batch threshold of csrc/gemm_route.h comes from
for b in 1 2 4 8 16 32; do
  for cfg in "0 1" "0 0" "1000000 0" "1000000 1"; do
    set -- $cfg
    ms=$(SE_AMD_GEMM_SMALL_M=$1 SE_AMD_FUSED_LN=$2 timeout -k 10 300 python bench.py --batch $b --steps 20 --warmup 3 --no-cpu-baseline --no-roofline 2>/dev/null | python -c "import sys,json; d=json.loads(sys.stdin.read()); print(round(d['ms_per_step'],3))")
    echo "batch $b SMALL_M=$1 FUSED_LN=$2: $ms ms"
  done
done

# on the GPU box: for each variant library run the bench and print its kernel table
cd /root/repo
OUT=${OUT:-bench_out}; mkdir -p "$OUT"  # where the bench lines and logs go
cp gpumd_amd/lib/libnepmi.so /tmp/libnepmi_product.so
for v in gpumd_amd/lib/variants/libnepmi_*.so; do
  name=$(basename $v .so); name=${name#libnepmi_}
  cp $v gpumd_amd/lib/libnepmi.so
  python bench.py --full --no-cpu-baseline $AB_ARGS > $OUT/ab_$name.json 2> $OUT/ab_$name.err
  python - $OUT/ab_$name.json $name <<'PY'
import json,sys
try:
    d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
    print("%-12s ms/step %.4f"%(sys.argv[2], d["ms_per_step"]), {k[:10]:round(v["avg_ms"],4) for k,v in d["kernels"].items() if k!="list_rebuild"})
except Exception as e:
    print(sys.argv[2], "ERR", e)
PY
done
cp /tmp/libnepmi_product.so gpumd_amd/lib/libnepmi.so

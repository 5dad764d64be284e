#!/bin/bash
# one GPU-box visit: the tests named on the command line (default: the convolution / fold / model tests), then the
# benchmark line with the kernel profile (--full, without the CPU baseline).  Logs land under $OUT (default out/gpu_check).
cd "$(dirname "$0")/.."
OUT=${OUT:-out/gpu_check}
mkdir -p $OUT
TESTS="${@:-tests/test_conv_gpu.py tests/test_conv_fold_gpu.py tests/test_bn_fold_gpu.py tests/test_model_gpu.py}"
timeout 1500 python -m pytest $TESTS -q -m gpu -x --no-header -p no:cacheprovider > $OUT/tests.log 2>&1
echo "pytest rc=$?" >> $OUT/tests.log
tail -40 $OUT/tests.log
timeout 600 python bench.py --full --no-cpu-baseline > $OUT/bench.json 2> $OUT/bench.err
echo "bench rc=$?"
cat $OUT/bench.json
tail -5 $OUT/bench.err

# GPU test driver used with gpurun (scripts/ travels with the snapshot, gpurun_out/ does not)
mkdir -p gpurun_out
timeout -k 10 700 python -m pytest tests/test_ops_gpu.py -m gpu -q -p no:cacheprovider > gpurun_out/ops.log 2>&1
rc=$?
rc2=0
rc3=0
rc4=0
rc5=0
rc6=0
echo "ops rc=$rc"; tail -3 gpurun_out/ops.log
if [ $rc -le 1 ]; then
  timeout -k 10 900 python -m pytest tests/test_net_gpu.py -m gpu -q -s -p no:cacheprovider > gpurun_out/net.log 2>&1
  rc2=$?
  echo "net rc=$rc2"; grep -E "HIP-vs-f64|gradient rel-L2|bf16 logits|passed|failed|FAILED" gpurun_out/net.log | tail -20
  if [ $rc2 -le 1 ]; then
    # every conv pass of the plan at its own shape, bitwise, with the batch-1 plan and the batch-16 source distances (measured:
    # 59-62 s on an MI355X box, most of it the CPU reference)
    # (its log is a temporary file: what a failure reports -- counts, first positions, planes -- is printed here)
    layers_log=$(mktemp)
    timeout -k 10 120 python -m pytest tests/test_conv_layers_gpu.py -m gpu -q -s -p no:cacheprovider > "$layers_log" 2>&1
    rc3=$?
    echo "layers rc=$rc3"; grep -E -A12 "not bitwise equal" "$layers_log" | cut -c1-200 | head -60
    grep -E "passed|failed|FAILED|Error" "$layers_log" | tail -20
    rm -f "$layers_log"
    if [ $rc3 -le 1 ]; then
      # every epilogue / pooling / up-sampling / head pass at its benchmark shape against float64 under derived bounds, and one
      # forward of the network block by block (measured: 19-20 s on an MI355X box, the float64 references included)
      epi_log=$(mktemp)
      timeout -k 10 45 python -m pytest tests/test_epilogue_layers_gpu.py -m gpu -q -s -p no:cacheprovider > "$epi_log" 2>&1
      rc4=$?
      echo "epilogue layers rc=$rc4"; grep -E -A8 "beyond the bound|not bitwise equal" "$epi_log" | cut -c1-200 | head -60
      grep -E "passed|failed|FAILED|Error" "$epi_log" | tail -20
      rm -f "$epi_log"
      if [ $rc4 -le 1 ]; then
        # the same conv passes at the second shipped configuration, 2 x 2 x 160^3 at width 2 (BASELINE.json configs[4]), bitwise
        # (batch 2; measured: 92-95 s on an MI355X box, most of it the CPU reference)
        c4_log=$(mktemp)
        timeout -k 10 190 python -m pytest tests/test_conv_layers_config4_gpu.py -m gpu -q -s -p no:cacheprovider > "$c4_log" 2>&1
        rc5=$?
        echo "config-4 layers rc=$rc5"; grep -E -A12 "not bitwise equal" "$c4_log" | cut -c1-200 | head -60
        grep -E "passed|failed|FAILED|Error" "$c4_log" | tail -20
        rm -f "$c4_log"
        if [ $rc5 -le 1 ]; then
          # and its epilogue / pooling / up-sampling / head passes and block-by-block forward (measured: 31-35 s on an MI355X box)
          c4e_log=$(mktemp)
          timeout -k 10 75 python -m pytest tests/test_epilogue_layers_config4_gpu.py -m gpu -q -s -p no:cacheprovider > "$c4e_log" 2>&1
          rc6=$?
          echo "config-4 epilogue layers rc=$rc6"; grep -E -A8 "beyond the bound|not bitwise equal" "$c4e_log" | cut -c1-200 | head -60
          grep -E "passed|failed|FAILED|Error" "$c4e_log" | tail -20
          rm -f "$c4e_log"
        else
          echo "config-4 layer run crashed or timed out (rc=$rc5): config-4 epilogue layer tests skipped"
        fi
      else
        echo "epilogue layer run crashed or timed out (rc=$rc4): config-4 layer tests skipped"
      fi
    else
      echo "layer run crashed or timed out (rc=$rc3): epilogue layer tests skipped"
    fi
  else
    echo "net run crashed or timed out (rc=$rc2): layer tests skipped"
  fi
else
  echo "ops run crashed or timed out (rc=$rc): net and layer tests skipped"
fi
rc7=0
if [ $rc -le 1 ] && [ $rc2 -le 1 ] && [ $rc3 -le 1 ] && [ $rc4 -le 1 ] && [ $rc5 -le 1 ] && [ $rc6 -le 1 ]; then
  # every 16-bit pass at the ends of its number range and on non-finite input (measured: 3 s + 7 s on an MI355X box)
  rng_log=$(mktemp)
  timeout -k 10 90 python -m pytest tests/test_conv_range_gpu.py tests/test_epilogue_range_gpu.py -m gpu -q -s -p no:cacheprovider > "$rng_log" 2>&1
  rc7=$?
  echo "range rc=$rc7"; grep -E -A10 "bit patterns differ|beyond the bound|that the plant reaches are finite" "$rng_log" | cut -c1-200 | head -60
  grep -E "passed|failed|FAILED|Error" "$rng_log" | tail -20
  rm -f "$rng_log"
fi
rc8=0
if [ $rc -le 1 ] && [ $rc2 -le 1 ] && [ $rc3 -le 1 ] && [ $rc4 -le 1 ] && [ $rc5 -le 1 ] && [ $rc6 -le 1 ] && [ $rc7 -le 1 ]; then
  # every conv pass of three non-cubic plans whose extents leave every tile ragged, bitwise (measured: 11-13 s on an MI355X box)
  rag_log=$(mktemp)
  timeout -k 10 90 python -m pytest tests/test_conv_layers_ragged_gpu.py -m gpu -q -s -p no:cacheprovider > "$rag_log" 2>&1
  rc8=$?
  echo "ragged layers rc=$rc8"; grep -E -A12 "not bitwise equal" "$rag_log" | cut -c1-200 | head -60
  grep -E "passed|failed|FAILED|Error" "$rag_log" | tail -20
  rm -f "$rag_log"
fi
rc9=0
if [ $rc -le 1 ] && [ $rc2 -le 1 ] && [ $rc3 -le 1 ] && [ $rc4 -le 1 ] && [ $rc5 -le 1 ] && [ $rc6 -le 1 ] && [ $rc7 -le 1 ] && [ $rc8 -le 1 ]; then
  # every epilogue / pooling / up-sampling / head pass of the same non-cubic volumes against float64 under derived bounds, one
  # forward block by block, and the heads' refusal of extents their levels do not divide (measured: 6-8 s, 10 s with start-up, on an MI355X box)
  rage_log=$(mktemp)
  timeout -k 10 60 python -m pytest tests/test_epilogue_layers_ragged_gpu.py -m gpu -q -s -p no:cacheprovider > "$rage_log" 2>&1
  rc9=$?
  echo "ragged epilogue layers rc=$rc9"; grep -E -A8 "beyond the bound|not bitwise equal" "$rage_log" | cut -c1-200 | head -60
  grep -E "passed|failed|FAILED|Error" "$rage_log" | tail -20
  rm -f "$rage_log"
fi
# exit status = the worst of the nine runs (a crash / timeout / GPU fault is a failure, not a skip)
[ $rc9 -gt $rc ] && rc=$rc9
[ $rc8 -gt $rc ] && rc=$rc8
[ $rc7 -gt $rc ] && rc=$rc7
[ $rc2 -gt $rc ] && rc=$rc2
[ $rc3 -gt $rc ] && rc=$rc3
[ $rc4 -gt $rc ] && rc=$rc4
[ $rc5 -gt $rc ] && rc=$rc5
[ $rc6 -gt $rc ] && rc=$rc6
exit $rc

# Round-2 profile set: bench line, rocprofv3 kernel trace of the same command, PMC passes (one counter
# group per run, --kernel-trace only), and the FETCH_SIZE calibration.  Outputs under gpurun_out/r02/;
# the summaries are copied into profiles/ by hand.
cd /tmp && export TMPDIR=/tmp
R=${GRAFT_REPO_ROOT:-/root/repo}
cd $R
O=gpurun_out/r02; rm -rf $O; mkdir -p $O
CMD="python bench.py --full --steps 200 --warmup 20 --no-cpu-baseline --no-throughputs --no-c4"
timeout 900 python bench.py --full > $O/bench.json 2> $O/bench.err
timeout 300 rocprofv3 --kernel-trace --stats -d $O/kt -o p -- $CMD > $O/kt.log 2>&1
python tools/rocpd_summary.py $(find $O/kt -name "*.db" | head -1) > $O/kernel_stats.txt 2>&1
i=0
for c in "FETCH_SIZE" "WRITE_SIZE" "TCC_HIT_sum TCC_MISS_sum" "SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAVES" \
         "SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_INSTS_SMEM SQ_INSTS_BRANCH" \
         "SQ_ACTIVE_INST_VALU SQ_THREAD_CYCLES_VALU SQ_WAVE_CYCLES SQ_WAIT_ANY" \
         "SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_BUSY_CYCLES GRBM_GUI_ACTIVE"; do
  i=$((i+1)); d=$O/pmc_$i; mkdir -p $d
  timeout 300 rocprofv3 --pmc $c --kernel-trace -d $d -o p -- python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-throughputs --no-c4 > $d/log.txt 2>&1
  echo "== pass $i ($c) rc=$?" >> $O/pmc.txt
  python tools/pmc_summary.py $(find $d -name "*.db" | head -1) 2>&1 | grep -E "k_pretok|k_tile_out" >> $O/pmc.txt
done
# FETCH_SIZE / WRITE_SIZE / TCC_MISS on known access patterns
i=0
for c in "FETCH_SIZE" "WRITE_SIZE" "TCC_MISS_sum TCC_HIT_sum" "TCC_EA0_RDREQ_sum TCC_EA0_RDREQ_32B_sum"; do
  i=$((i+1)); d=$O/cal_$i; mkdir -p $d
  timeout 200 rocprofv3 --pmc $c --kernel-trace -d $d -o p -- _ab/calib_fetch > $d/log.txt 2>&1
  echo "== calibration pass $i ($c) rc=$?" >> $O/calib.txt
  python tools/pmc_summary.py $(find $d -name "*.db" | head -1) 2>&1 >> $O/calib.txt
done
head -1 $O/cal_1/log.txt >> $O/calib.txt
rm -rf $O/kt $O/pmc_* $O/cal_*/*.db 2>/dev/null
ls -la $O

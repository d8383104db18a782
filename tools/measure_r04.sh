# round-4 measurement set (run on the GPU box from the repo root): bash tools/measure_r04.sh <tag> [quick]
set -x
cd $GRAFT_REPO_ROOT
T=${1:-r04}
O=gpurun_out/$T; mkdir -p $O
line() { python -c "import sys,json; r=json.loads([l for l in sys.stdin if l.startswith('{')][-1]); c=r['config']; print('$1', 'scenes/s', round(r['value'],2), 'ms/step', round(r['ms_per_step'],2), 'ref-order', round(r.get('value_reference_order') or 0,2), 'B', c.get('scenes_per_gpu'), 'voxels', c['voxels_per_scene'], {k:round(v,2) for k,v in c.items() if k.startswith('step_ms')})"; }
# 1. default bench line (with cpu baseline incl. the unscaled full-size pass)
python bench.py --full > $O/bench.json 2> $O/bench.err
# 2. step time vs scene size, scenes per GPU, rotation
for v in 20000 80000 150000 300000; do python bench.py --full --no-cpu-baseline --voxels $v --steps 20 --warmup 5 2>/dev/null | line voxels=$v; done > $O/step_vs_scene_size.txt
for B in 1 2 4 8; do python bench.py --no-cpu-baseline --no-reference-order --steps 12 --warmup 4 --scenes-per-gpu $B 2>/dev/null | tee $O/bench_B$B.json | line B=$B; done > $O/scenes_per_gpu.txt
python bench.py --no-cpu-baseline --no-reference-order --steps 32 --warmup 8 --rotate 8 2>/dev/null | tee $O/bench_rotate8.json | line rotate8 >> $O/scenes_per_gpu.txt
# 3. host vs device (threaded prefetch on / off; 150 k and 20 k voxels)
for v in 150000 20000; do for t in 1 0; do echo -n "voxels=$v prefetch_thread=$t: "; USC3D_PREFETCH_THREAD=$t python tools/host_vs_device.py --no-cpu-baseline --voxels $v 2>/dev/null | tail -n 1; done; done > $O/host_vs_device.txt
for p in 1 0; do echo -n "voxels=150000 backbone_program=$p prefetch_thread=0: "; USC3D_BACKBONE_PROGRAM=$p USC3D_PREFETCH_THREAD=0 python tools/host_vs_device.py --no-cpu-baseline 2>/dev/null | tail -n 1; done >> $O/host_vs_device.txt
# 4. two ranks (gloo, sharing this box's one device: the code path, not a scaling number) drawing scenes through the sampler
python bench.py --gpus 2 --dist-backend gloo --rotate 4 --steps 8 --warmup 2 --no-cpu-baseline --no-reference-order > $O/bench_2rank_gloo_rotate.json 2> $O/bench_2rank.err
python bench.py --gpus 2 --dist-backend gloo --rotate 4 --bucket-window 1 --steps 8 --warmup 2 --no-cpu-baseline --no-reference-order > $O/bench_2rank_gloo_rotate_plain.json 2>> $O/bench_2rank.err
[ "$2" = quick ] && exit 0
# 5. kernel stats of the bench command
(cd /tmp && export TMPDIR=/tmp && rocprofv3 --kernel-trace --stats --output-format csv -d $GRAFT_REPO_ROOT/$O/prof -- python $GRAFT_REPO_ROOT/bench.py --no-cpu-baseline --no-reference-order > $GRAFT_REPO_ROOT/$O/prof.log 2>&1)
python tools/prof_summary.py $O/prof 90 > $O/kernel_stats_summary.txt
cp $(ls $O/prof/*/*kernel_stats.csv | head -1) $O/kernel_stats.csv
# 6. PMC traffic passes (separate runs, counters only with kernel-trace)
(cd /tmp && export TMPDIR=/tmp && rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $GRAFT_REPO_ROOT/$O/pmc_fetch -- python $GRAFT_REPO_ROOT/bench.py --steps 2 --warmup 1 --no-cpu-baseline --no-reference-order > /dev/null 2>&1)
(cd /tmp && export TMPDIR=/tmp && rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d $GRAFT_REPO_ROOT/$O/pmc_write -- python $GRAFT_REPO_ROOT/bench.py --steps 2 --warmup 1 --no-cpu-baseline --no-reference-order > /dev/null 2>&1)
for k in gather_gemm wgrad; do python tools/pmc_summary.py $O/pmc_fetch $k; python tools/pmc_summary.py $O/pmc_write $k; done > $O/pmc_traffic_raw.txt
rm -rf $O/pmc_fetch $O/pmc_write $O/prof
# 7. HBM report, ncut bench, conv per shape
python tools/hbm_report.py > $O/hbm_bound_kernels.txt 2>/dev/null
python bench.py --mode ncut --full > $O/bench_ncut.json 2>/dev/null
for k in 1 4 16 24; do python bench.py --mode ncut --scenes $k --no-cpu-baseline --steps 2 --warmup 1 2>/dev/null | python -c "import sys,json; r=json.loads(sys.stdin.readline()); print('ncut scenes in flight', r['scenes_in_flight'], round(r['value'],2), 'scenes/s', round(r['ms_per_step'],1), 'ms/scene', r['config']['masks'], 'masks')"; done > $O/ncut_scenes_in_flight.txt
USC3D_PROF_SHAPES=1 python tools/conv_report.py > $O/conv_per_shape.txt 2>/dev/null
ls -la $O

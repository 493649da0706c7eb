#!/bin/bash
# The measurements behind profiles/hessian_image/ (the Hessian image of csrc/bq_h52.h against the parent commit).  On the GPU box, from
# the root of this tree, with a built tree of the parent commit beside it:
#   tools/profile_hessian_image.sh OUTDIR PARENT_TREE STEP...
# steps, each a set of fresh processes under its own time limit:
#   headline_ab  python bench.py --gpus 1 --steps 50 --warmup 5, alternating parent / this build, three runs each
#   c2_ab        the same with --config c2
#   c4_c5        --config c4 and --config c5, one run a side (they get no image)
#   outputs      --dump-outputs of the headline and of c2 on both builds, compared byte for byte (x, g, stats)
#   counters     FETCH_SIZE of the tile kernel on both builds: rocprofv3 --pmc alone, no tracing in the same run
#   setup        the image's build time, its candidates' times and the break-even product count at the headline and at c2
# OUTDIR is a directory of its own (created).  Every bench line lands in OUTDIR/<step>_<build>_<k>.json; tools/hessian_image_ab.py turns them into the *_ab.json files.
# A process that ends on a signal or a time limit ends the script: nothing more is started on the GPU after it.
set -o pipefail
dir=$1; parent=$2; shift 2
here=$(pwd)
case $dir in /*) out=$dir ;; *) out=$here/$dir ;; esac
mkdir -p "$out"
export TMPDIR=/tmp
run() {   # run LIMIT TREE OUTFILE command...
    limit=$1; tree=$2; file=$3; shift 3
    (cd "$tree" && timeout -k 10 "$limit" "$@") > "$file" 2> "$file.err"
    rc=$?
    if [ $rc -ne 0 ]; then
        echo "[hessian_image] $file rc=$rc"; tail -n 5 "$file.err"
        if [ $rc -ge 124 ]; then exit $rc; fi
        return $rc
    fi
    rm -f "$file.err"
}
line() { tail -n 1 "$1" | cut -c1-400; }
for step in "$@"; do
  start=$(date +%s)
  case $step in
    headline_ab|c2_ab)
      cfg=(); [ $step = c2_ab ] && cfg=(--config c2)
      for k in 1 2 3; do
        run 240 "$parent" "$out/${step}_parent_$k.json" python bench.py --gpus 1 --steps 50 --warmup 5 --line full "${cfg[@]}" || exit 1
        run 240 "$here" "$out/${step}_image_$k.json" python bench.py --gpus 1 --steps 50 --warmup 5 --line full "${cfg[@]}" || exit 1
      done ;;
    c4_c5)
      for c in c4 c5; do
        run 400 "$parent" "$out/${c}_parent_1.json" python bench.py --gpus 1 --steps 50 --warmup 5 --line full --config $c || exit 1
        run 400 "$here" "$out/${c}_image_1.json" python bench.py --gpus 1 --steps 50 --warmup 5 --line full --config $c || exit 1
      done ;;
    outputs)
      : > "$out/outputs_compare.txt"
      for c in headline c2; do
        run 240 "$parent" "$out/dump_${c}_parent.json" python bench.py --gpus 1 --steps 50 --warmup 5 --config $c --dump-outputs "$out/dump_${c}_parent" || exit 1
        run 240 "$here" "$out/dump_${c}_image.json" python bench.py --gpus 1 --steps 50 --warmup 5 --config $c --dump-outputs "$out/dump_${c}_image" || exit 1
        for a in x g stats; do
          if cmp -s "$out/dump_${c}_parent/$a.npy" "$out/dump_${c}_image/$a.npy"; then r=identical; else r=DIFFERENT; fi
          echo "$c $a.npy $(stat -c %s "$out/dump_${c}_image/$a.npy") bytes $(sha256sum < "$out/dump_${c}_image/$a.npy" | cut -c1-16) $r" >> "$out/outputs_compare.txt"
        done
        rm -rf "$out/dump_${c}_parent" "$out/dump_${c}_image" "$out/dump_${c}_parent.json" "$out/dump_${c}_image.json"
      done
      cat "$out/outputs_compare.txt" ;;
    counters)
      for b in parent image; do
        tree=$here; [ $b = parent ] && tree=$parent
        run 400 "$tree" "$out/pmc_${b}.json" rocprofv3 --pmc FETCH_SIZE --output-format csv -d "$out/pmc_$b" -- python3 bench.py --gpus 1 --steps 10 --warmup 2 || exit 1
        f=$(find "$out/pmc_$b" -name '*counter_collection.csv' | head -1)
        python3 tools/hessian_image_ab.py fetch "$f" "$out/pmc_fetch_size_$b.json" || exit 1
        rm -rf "$out/pmc_$b"   # the per-dispatch CSV is large: the summary is kept
      done ;;
    setup)
      run 300 "$here" "$out/setup_cost.json" python tools/hessian_image_ab.py setup headline c2 || exit 1
      cat "$out/setup_cost.json" ;;
    *) echo "[hessian_image] unknown step $step" ;;
  esac
  echo "[hessian_image] $step done in $(( $(date +%s) - start )) s"
done
python3 tools/hessian_image_ab.py collate "$out"

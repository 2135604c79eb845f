# developer tool: timing-only ablations of fwd_fused_kernel (ALEPPO_FF_ABLATE).  Needs the ablation build of the library:
# make ABLATIONS=1 in ale-libtorch-ppo_amd/csrc (after a make clean); the default build has neither the variants nor the
# variable.
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
for a in 0 1 2 4 8 16; do
  ALEPPO_FF_ABLATE=$a ALEPPO_FWD_FUSED=1 rocprofv3 --kernel-trace --output-format csv -d gpurun_out/ffa_$a -- python3 tests/tools/upd_time.py 3 > gpurun_out/ffa_$a.log 2>&1 || exit 1
  python3 - $a <<'PY'
import csv,glob,sys
f=glob.glob("gpurun_out/ffa_%s/**/*kernel_trace.csv"%sys.argv[1],recursive=True)[0]
d=[(int(r["End_Timestamp"])-int(r["Start_Timestamp"]))/1e3 for r in csv.DictReader(open(f)) if "fwd_fused" in r["Kernel_Name"]]
d.sort(); print("ablate",sys.argv[1],"median us",d[len(d)//2],"n",len(d))
PY
done

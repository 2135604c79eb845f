# developer tool: timing-only ablations of conv_bwd_fused_kernel (ALEPPO_CB_ABLATE), kernel alone on one stream
# (UPD_SERIAL=1: upd_time.py sets ALEPPO_OPT_SERIAL_UPDATE).  Needs the ablation build of the library: make ABLATIONS=1 in
# ale-libtorch-ppo_amd/csrc (after a make clean); the default build has neither the variants nor the variable.
# usage, from the repository root: bash tests/tools/cbabl.sh OUTDIR (as tests/tools/ab.sh: traces and logs go under OUTDIR)
OUT=${1:?usage: bash tests/tools/cbabl.sh OUTDIR}; mkdir -p $OUT
for a in 0 1 2 4 8 16 31; do
  ALEPPO_CB_ABLATE=$a UPD_SERIAL=1 ALEPPO_BWD_FUSED=2 rocprofv3 --kernel-trace --output-format csv -d $OUT/cba_$a -- python3 tests/tools/upd_time.py 3 > $OUT/cba_$a.log 2>&1 || exit 1
  python3 - $a $OUT <<'PY'
import csv,glob,sys
f=glob.glob("%s/cba_%s/**/*kernel_trace.csv"%(sys.argv[2],sys.argv[1]),recursive=True)[0]
d=[(int(r["End_Timestamp"])-int(r["Start_Timestamp"]))/1e3 for r in csv.DictReader(open(f)) if "conv_bwd_fused" in r["Kernel_Name"]]
d.sort(); print("ablate",sys.argv[1],"median us (alone, one stream)",d[len(d)//2],"n",len(d))
PY
done

"""Per-stage shader clocks of the window chain's assemble-only launch (S24 / S24D), and, with a -DMJH_COLLIDE_PROBE library, of the
three parts of its collision stage: python tools/collide_stage_profile.py [nenv] [settle]"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import mujoco_sim_amd as ms
from mujoco_sim_amd import capi
cfg = "s24"
nenv = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
settle = int(sys.argv[2]) if len(sys.argv) > 2 else 400
m = ms.scene("s24"); e = ms.Engine(m, nenv); e.load_s24()
e.step(settle); e.synchronize()
names = ["", "load state", "FK + geoms", "COM/cdof/CRBA", "factor", "collision", "row headers", "J rows + params", "B, A_c, schedule",
         "vel stage (RNE, aref)", "controller/inverse", "smooth acc", "warmstart + AR", "PGS sweeps", "checkAcc + integrate", "store"]
out = np.zeros(20)
for rep in range(3):
    capi.load().mjh_debug_stage_cycles(e.h, 8, capi.dptr(out))
st = e.get_stats()
print("COLLIDE_STAGES", cfg, "nenv", nenv, "mean ncon %.1f nefc %.1f" % (st[:, 0].mean(), st[:, 1].mean()))
last = max(out[:16])
prev = 0
for k in range(1, 16):
    if out[k] == 0: continue
    print(f"{k:2d} {names[k]:22s} +{out[k]-prev:10.0f} ticks  {100*(out[k]-prev)/last:5.1f} %   cum {out[k]:10.0f}")
    prev = out[k]
if out[16] > 0:
    c0, c1 = out[4], out[5]
    parts = [("narrow phase (per lane)", out[16] - c0), ("scan of the counts", out[17] - out[16]), ("emit", out[18] - out[17]), ("rest of the stage", c1 - out[18])]
    for nm, v in parts:
        print(f"   collision: {nm:24s} {v:10.0f} ticks  {100*v/(c1-c0):5.1f} % of the stage")

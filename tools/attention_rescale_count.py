"""How often the split attention kernel's rescale branch is taken (csrc/attention.hip, AT_TAU) on the data of one bench.py step: SuperPoint + SuperGlue
on 32 synthetic pairs (bench.py's first batch, seeds 0 .. 31, 720 x 540), 18 attention launches.  Per launch: the tiles executed (one per wavefront
and 32 keys), the tiles that rescaled, and the tiles that WOULD have rescaled with the running maximum as the reference (the kernel before AT_TAU;
both are counted on the same scores in one launch).  From a MEASUREMENT build of the whole library with attention.hip compiled -DAT_PROF
(tools/ubench/libmfr_hip_att_prof.so; build it on the CPU box: `python tools/attention_rescale_count.py --build`); the product library carries no counter.
    python tools/attention_rescale_count.py [out.json]"""
import ctypes as C
import glob
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CSRC = os.path.join(ROOT, "map-free-reloc_amd", "csrc")
SO = os.path.join(ROOT, "tools", "ubench", "libmfr_hip_att_prof.so")
if "--build" in sys.argv:
    # the product objects of every other translation unit (csrc/_build, `make`), attention.hip again with the counters
    objs = [o for o in sorted(glob.glob(os.path.join(CSRC, "_build", "*.o"))) if os.path.basename(o) != "attention.o"]
    assert objs, "build the product library first (make -C map-free-reloc_amd/csrc)"
    prof_o = os.path.join(ROOT, "tools", "ubench", "attention_prof.o")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=fast", "-DAT_PROF",
                           "-I" + os.path.join(ROOT, "include"), "-c", os.path.join(CSRC, "attention.hip"), "-o", prof_o])
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-shared", "-fPIC", "-o", SO, prof_o] + objs)
    print("built", SO)
    sys.exit(0)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import mapfree_reloc_amd as mfr  # noqa: E402
from mapfree_reloc_amd import images as IM  # noqa: E402

mfr._lib.SO_PATH = SO
lib = mfr._lib.load(require_gpu=True)
from mapfree_reloc_amd.pipeline import SuperGluePnPPipeline  # noqa: E402

SLOTS = 64
dev = "cuda:0"
sb = IM.synthetic_batch(list(range(32)), 720, 540)
d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in sb.items() if isinstance(v, np.ndarray)}
pipe = SuperGluePnPPipeline(dev, seed=0)
buf, n = (C.c_uint * (SLOTS * 3))(), C.c_int()
pipe(d["images"], d["depth0"], d["K0"], d["K1"], d["pair_ids"])
assert lib.mfr_sg_attention_profile(buf, C.byref(n)) == 0              # (the first step: discarded with its lazy initialisation)
out = pipe(d["images"], d["depth0"], d["K0"], d["K1"], d["pair_ids"])
assert lib.mfr_sg_attention_profile(buf, C.byref(n)) == 0
assert 0 < n.value <= SLOTS, n.value
rows = [{"launch": i, "cross": bool(pipe.sg.layers[i]["cross"]), "tiles": buf[3 * i], "rescaled": buf[3 * i + 1], "rescaled_running_max": buf[3 * i + 2]} for i in range(n.value)]
tot = [sum(r[k] for r in rows) for k in ("tiles", "rescaled", "rescaled_running_max")]
res = {"what": "tiles (per wavefront: 32 queries x 32 keys) of the attention launches of one SuperPoint + SuperGlue step, 32 pairs (bench.py batch 0)",
       "tau": 14, "launches": n.value, "mean_keypoints_per_image": float(out["n_kpts"].float().mean()) if "n_kpts" in out else None,
       "tiles": tot[0], "share_rescaled": round(tot[1] / tot[0], 4), "share_rescaled_running_max": round(tot[2] / tot[0], 4), "per_launch": rows}
print(json.dumps({k: v for k, v in res.items() if k != "per_launch"}))
for r in rows:
    print(f'{r["launch"]:3d} {"cross" if r["cross"] else "self ":5s} tiles {r["tiles"]:8d}  rescaled {r["rescaled"] / r["tiles"]:.4f}  with a running maximum {r["rescaled_running_max"] / r["tiles"]:.4f}')
if sys.argv[-1].endswith(".json"):
    json.dump(res, open(sys.argv[-1], "w"), indent=1)

"""Workspace sizes of the pose solvers, pinned: a caller sizes its buffer once with mfr_*_workspace_bytes and the library carves it
(csrc/wave_dev.h WsCarver), so a size that moves is an ABI change.  The literals are what the library returned before the layouts were
restated as carver takes.  Host functions: no GPU needed."""
import itertools

import mapfree_reloc_amd as mfr

BS, NS, ITERS = (1, 3, 32), (1, 255, 256, 2048), (1, 1000, 4096)
HWS = ((1, 1), (48, 64), (540, 720))
PAIRS = (1, 3, 32, 255, 256, 2048)

# itertools.product(BS, NS, ITERS) order
PNP = (
    2304, 6144, 18432, 13568, 17408, 29696, 13568, 17408, 29696, 101376, 105216, 117504,
    2304, 14080, 51200, 38656, 50432, 87552, 38656, 50432, 87552, 302080, 313856, 350976,
    4864, 132608, 528896, 402944, 530688, 926976, 404224, 531968, 928256, 3214080, 3341824, 3738112,
)
EMAT = (
    3072, 741888, 3032320, 11520, 750336, 3040768, 11520, 750336, 3040768, 77824, 816640, 3107072,
    4608, 2221568, 9094400, 32000, 2248960, 9121792, 32000, 2248960, 9121792, 230912, 2447872, 9320704,
    25856, 23681792, 96995072, 326400, 23982336, 97295616, 327424, 23983360, 97296640, 2449152, 26105088, 99418368,
)
PROCRUSTES = (
    2048, 13824, 50688, 14592, 26368, 63232, 14592, 26368, 63232, 107776, 119552, 156416,
    2048, 37632, 148992, 41216, 76800, 188160, 41216, 76800, 188160, 320768, 356352, 467712,
    6656, 390144, 1579008, 429312, 812800, 2001664, 430848, 814336, 2003200, 3412736, 3796224, 4985088,
)
# itertools.product(BS, NS) order
SCALE = (
    1024, 2816, 2816, 17152, 1024, 6912, 6912, 49920, 1024, 66048, 66304, 526592,
)
# itertools.product(BS, HWS) order
ICP = (
    1024, 76032, 9538304, 1792, 227328, 28614400, 11520, 2417920, 305215488,
)
ABS_POSE = (
    256, 768, 8192, 65280, 65536, 524288,
)


def test_solver_workspace_sizes_are_pinned():
    lib = mfr._lib.load()
    grid = list(itertools.product(BS, NS, ITERS))
    assert tuple(lib.mfr_pnp_workspace_bytes(*a) for a in grid) == PNP
    assert tuple(lib.mfr_emat_workspace_bytes(*a) for a in grid) == EMAT
    assert tuple(lib.mfr_procrustes_workspace_bytes(*a) for a in grid) == PROCRUSTES
    assert tuple(lib.mfr_scale_workspace_bytes(B, N) for B, N in itertools.product(BS, NS)) == SCALE
    assert tuple(lib.mfr_procrustes_icp_workspace_bytes(B, H, W) for B, (H, W) in itertools.product(BS, HWS)) == ICP
    assert tuple(lib.mfr_abs_pose_workspace_bytes(P) for P in PAIRS) == ABS_POSE

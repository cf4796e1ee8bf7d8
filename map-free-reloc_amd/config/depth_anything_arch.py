"""The architectures of Depth Anything V2 (DINOv2 ViT-S / B / L behind a DPT head) as plain values: the presets behind the config's DA.ENCODER and the
defaults of nets/depth_anything.check_arch.  No imports: building a config must not load the network code.

POS_GRID is the side of the square grid the position embeddings were trained on (518 / 14 = 37); MAX_DEPTH / METRIC are the head's output convention:
the metric checkpoints end in max_depth * sigmoid (Hypersim: 20, Virtual KITTI: 80), the relative ones in a ReLU."""
_COMMON = dict(PATCH=14, POS_GRID=37, HEAD_WIDTH=32, MAX_DEPTH=20.0, METRIC=True)

PRESETS = dict(
    vits=dict(VIT_WIDTH=384, VIT_LAYERS=12, VIT_HEADS=6, VIT_MLP=1536, TAPS=(2, 5, 8, 11), REASSEMBLE_WIDTH=384, NECK_SIZES=(48, 96, 192, 384),
              FUSION_WIDTH=64, **_COMMON),
    vitb=dict(VIT_WIDTH=768, VIT_LAYERS=12, VIT_HEADS=12, VIT_MLP=3072, TAPS=(2, 5, 8, 11), REASSEMBLE_WIDTH=768, NECK_SIZES=(96, 192, 384, 768),
              FUSION_WIDTH=128, **_COMMON),
    vitl=dict(VIT_WIDTH=1024, VIT_LAYERS=24, VIT_HEADS=16, VIT_MLP=4096, TAPS=(4, 11, 17, 23), REASSEMBLE_WIDTH=1024, NECK_SIZES=(256, 512, 1024, 1024),
              FUSION_WIDTH=256, **_COMMON),
)
ARCH = PRESETS["vits"]

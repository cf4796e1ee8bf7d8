"""The architecture of DPT-Hybrid (dpt_hybrid-midas / dpt_hybrid_kitti / dpt_hybrid_nyu) as plain values: the defaults of the config's DPT.ARCH node and of
nets/dpt.check_arch.  No imports: building a config must not load the network code."""
ARCH = dict(BIT_DEPTHS=(3, 4, 9), BIT_HIDDEN_SIZES=(256, 512, 1024), BIT_EMBEDDING_SIZE=64, NUM_GROUPS=32, VIT_WIDTH=768, VIT_LAYERS=12, VIT_HEADS=12,
            VIT_MLP=3072, NECK_SIZES=(256, 512, 768, 768), FUSION_WIDTH=256, TAPS=(2, 5, 8, 11), PATCH=16)

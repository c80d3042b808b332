"""Small relatives of Model B for the fused BN-CNN plan (train/bncnn.py): each case exists for branches of the
host planners (csrc/kernels/bncnn.hip ``conv_fwd_plan`` / ``conv_bwd_plan``) and of the kernels that Model B's
three square, equal-stride, kernel-divisible-by-stride layers never take.  ``plan`` lists, per conv block, the
planner outputs that prove the branch is taken — tests/test_bncnn_family_gpu.py asserts them, so a later
planner change cannot silently move a case off its branch:

    fwd = (ks, msplit)                                    tde_bncnn_conv_fwd_cfg out[1:3]
    bwd = (wgrad items, dgrad items, wg_split, ksd, staged floats)   tde_bncnn_conv_bwd_plan out[1:6]

(dgrad items = mtd * nnt * ksd; the first block has no input gradient: dgrad items 0, staged 0.)  ``derived``
holds (ncls, nnt) of the blocks with an input gradient: ncls = sh * sw stride classes, nnt = ceil(ncls * C / 16)
N tiles of the class-stacked weights.

No GPU marker: the models build and match on the CPU (tests/test_bncnn_oracle.py)."""
from __future__ import annotations

import torch

# conv block: (filters, (kh, kw), (sh, sw), padding, bn flags);  bn flags: dict(scale, center[, epsilon, momentum])
_TT = dict(scale=True, center=True)
_TF = dict(scale=True, center=False)
_FT = dict(scale=False, center=True)
_FF = dict(scale=False, center=False)
_ODD = dict(scale=True, center=True, epsilon=1e-5, momentum=0.9)

CASES = {
    # second block: ncls = 4 with k = 5 at stride 2 (taps past the kernel in the class stack), Co = 17 (the
    # second N tile holds one live column), 2 x 1 output pixels, H != W; K = 34 (scalar dense form), Dp = 32
    # with 15 dead columns.  The stack (6144 floats, msplit = 1) needs 6 rows of forward threads.
    "A": dict(input=(13, 11, 3), convs=[(5, (3, 3), (2, 2), "same", _TT), (17, (5, 5), (2, 2), "valid", _TT)],
              D=17, NC=10, bnd=_TT, softmax=True, batch=24,
              plan=[dict(fwd=(1, 2), bwd=(4, 0, 2, None, 0)), dict(fwd=(4, 1), bwd=(8, 8, 1, 4, 6144))],
              derived=[None, (4, 2)]),
    # strides 1x2 (image layer) and 2x1 (ncls = 2 on a layer with an input gradient), non-square kernels,
    # Co = 16 exactly, pl = 1 / pr = 2 on the first and pl = 0 / pr = 1 on the second block, a 1x1 conv
    # (ncls = 1, nnt = 1), L = 3, K = 270 (K % 4 == 2), 16 classes; no beta anywhere
    "B": dict(input=(12, 10, 2), convs=[(16, (3, 5), (1, 2), "same", _TF), (7, (4, 2), (2, 1), "same", _TF),
                                        (9, (1, 1), (1, 1), "valid", _TF)],
              D=200, NC=16, bnd=_TF, softmax=True, batch=24,
              plan=[dict(fwd=(1, 2), bwd=(6, 0, 3, None, 0)), dict(fwd=(4, 2), bwd=(16, 6, 2, 1, 1024)),
                    dict(fwd=(1, 2), bwd=(2, 2, 2, 1, 256))],
              derived=[None, (2, 2), (1, 1)]),
    # second block: nnt = 4 (the limit: 4 classes x 16 channels), ksd = 2, Co = 32; D = 256, 2 classes;
    # epsilon 1e-5 and momentum 0.9 on every BN
    "C": dict(input=(9, 9, 1), convs=[(16, (3, 3), (1, 1), "same", _ODD), (32, (3, 3), (2, 2), "same", _ODD)],
              D=256, NC=2, bnd=_ODD, softmax=True, batch=24,
              plan=[dict(fwd=(1, 2), bwd=(5, 0, 5, None, 0)), dict(fwd=(4, 2), bwd=(9, 16, 1, 2, 8192))],
              derived=[None, (4, 4)]),
    # L = 1, C = Co = 1, pt = 1 / pb = 2 on the image layer, D below one tile; a conv BN with neither gamma
    # nor beta
    "D": dict(input=(8, 8, 1), convs=[(1, (4, 4), (1, 1), "same", _FF)],
              D=8, NC=10, bnd=_FT, softmax=True, batch=24,
              plan=[dict(fwd=(1, 2), bwd=(4, 0, 4, None, 0))],
              derived=[None]),
    # all-valid, msplit = 1 on both layers, an even kernel, K = 45; the logits head; BN flags mixed per layer
    "F": dict(input=(9, 9, 2), convs=[(5, (3, 3), (2, 2), "valid", _TF), (5, (2, 2), (1, 1), "valid", _FT)],
              D=16, NC=10, bnd=_TT, softmax=False, batch=24,
              plan=[dict(fwd=(1, 1), bwd=(2, 0, 1, None, 0)), dict(fwd=(1, 1), bwd=(2, 1, 1, 1, 512))],
              derived=[None, (1, 1)]),
    # second block: the class-stacked weights (Kdp * NP = 224 * 64 = 14336 floats) do not fit the prefetch
    # registers (11264) while K * Co = 9600 does: wgather == 0, the backward gathers from the HWIO kernel
    "I": dict(input=(9, 9, 1), convs=[(16, (3, 3), (1, 1), "same", _TT), (24, (5, 5), (2, 2), "same", _TT)],
              D=32, NC=10, bnd=_TT, softmax=True, batch=24,
              plan=[dict(fwd=(1, 2), bwd=(5, 0, 5, None, 0)), dict(fwd=(8, 2), bwd=(25, 16, 1, 2, 0))],
              derived=[None, (4, 4)]),
    # strides 1x2 on a layer WITH an input gradient (case B has them on the image layer only): ncls = 2 along
    # the width, a 2x3 kernel (kw = 3 not divisible by sw = 2), pl = 0 / pr = 1, H != W
    "G": dict(input=(10, 12, 2), convs=[(4, (3, 3), (1, 1), "same", _FT), (6, (2, 3), (1, 2), "same", _FT)],
              D=24, NC=10, bnd=_FT, softmax=True, batch=24,
              plan=[dict(fwd=(1, 2), bwd=(14, 0, 7, None, 0)), dict(fwd=(1, 2), bwd=(6, 4, 3, 1, 512))],
              derived=[None, (2, 1)]),
}


def build(tde, case, rate=None, opt=None, seed=3):
    """The compiled, built model of CASES[case] with non-trivial gammas, betas and moving statistics."""
    c = CASES[case] if isinstance(case, str) else case
    L = tde.layers if hasattr(tde, "layers") else tde.keras.layers
    ls = []
    for i, (filters, ks, strides, padding, bn) in enumerate(c["convs"]):
        kw = dict(input_shape=c["input"]) if i == 0 else {}
        ls += [L.Conv2D(filters=filters, kernel_size=ks, strides=strides, padding=padding, use_bias=False, **kw),
               L.BatchNormalization(**bn), L.Activation("relu")]
    ls += [L.Flatten(), L.Dense(c["D"], use_bias=False), L.BatchNormalization(**c["bnd"]), L.Activation("relu")]
    if rate is not None:
        ls.append(L.Dropout(rate))
    ls.append(L.Dense(c["NC"], activation="softmax" if c["softmax"] else None))
    m = tde.Sequential(ls)
    loss = "sparse_categorical_crossentropy" if c["softmax"] else \
        tde.losses.SparseCategoricalCrossentropy(from_logits=True)
    m.compile(loss=loss, optimizer=opt or tde.optimizers.SGD(0.01), metrics=["accuracy"])
    m.build()
    randomize_bn(m, seed)
    return m


def randomize_bn(m, seed=3):
    """gamma in [0.5, 1.5), beta in [-0.1, 0.1), moving mean in [-0.5, 0.5), moving variance in [0.5, 1.5)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    st = m._store
    for n in st.names():
        leaf = n.rsplit("/", 1)[-1]
        v = st.view(n)
        r = torch.rand(v.shape, generator=g)
        if leaf == "gamma":
            v.copy_((r + 0.5).to(v.device))
        elif leaf == "beta":
            v.copy_(((r - 0.5) * 0.2).to(v.device))
        elif leaf == "moving_mean":
            v.copy_((r - 0.5).to(v.device))
        elif leaf == "moving_variance":
            v.copy_((r + 0.5).to(v.device))


def data(case, B, seed, device="cpu"):
    c = CASES[case] if isinstance(case, str) else case
    H, W, C = c["input"]
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.rand(B, H * W * C, generator=g).to(device)
    y = torch.randint(0, c["NC"], (B,), generator=g).int().to(device)
    return x, y


def model_b(tde, rate=0.0, opt=None):
    """Model B (mnist_keras_distributed.py:79-109) with non-trivial BN betas."""
    L = tde.layers if hasattr(tde, "layers") else tde.keras.layers
    m = tde.Sequential([
        L.Reshape(input_shape=(28 * 28,), target_shape=(28, 28, 1)),
        L.Conv2D(filters=6, kernel_size=3, padding="same", use_bias=False),
        L.BatchNormalization(scale=False, center=True),
        L.Activation("relu"),
        L.Conv2D(filters=12, kernel_size=6, padding="same", use_bias=False, strides=2),
        L.BatchNormalization(scale=False, center=True),
        L.Activation("relu"),
        L.Conv2D(filters=24, kernel_size=6, padding="same", use_bias=False, strides=2),
        L.BatchNormalization(scale=False, center=True),
        L.Activation("relu"),
        L.Flatten(),
        L.Dense(200, use_bias=False),
        L.BatchNormalization(scale=False, center=True),
        L.Activation("relu"),
        L.Dropout(rate),
        L.Dense(10, activation="softmax"),
    ])
    m.compile(loss="sparse_categorical_crossentropy", optimizer=opt or tde.optimizers.SGD(0.01), metrics=["accuracy"])
    m.build()
    # non-trivial BN betas / moving statistics
    g = torch.Generator(device="cpu").manual_seed(3)
    for n in m._store.names():
        if n.endswith("/beta"):
            v = m._store.view(n)
            v.copy_((torch.rand(v.shape, generator=g) - 0.5).to(v.device) * 0.2)
    return m


def model_b_data(B, seed, device="cpu"):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.rand(B, 784, generator=g).to(device)
    y = torch.randint(0, 10, (B,), generator=g).int().to(device)
    return x, y

"""DepthwiseConv2D / SeparableConv2D on the host: the layers' reference forward against a nested-loop float64
convolution written from the definition, their Keras shapes / weights / configs, the refusals, the zoo model on
the reference plan and its SavedModel graph."""
import numpy as np
import pytest
import torch

import tensorflow_distributed_example_amd as tde
from tensorflow_distributed_example_amd.models import layers as L

CASES = [  # B, H, W, C, dm, kh, kw, sh, sw, padding
    (2, 5, 5, 1, 1, 3, 3, 1, 1, "same"),
    (2, 9, 7, 3, 2, 3, 3, 1, 1, "valid"),
    (2, 16, 14, 8, 1, 3, 3, 2, 2, "same"),
    (1, 11, 13, 4, 1, 3, 5, 2, 1, "same"),
]


def _loops(x, w, sh, sw, padding):
    """y[b,oh,ow,c*dm+m] = sum_{i,j} x[b, oh*sh-pt+i, ow*sw-pl+j, c] * w[i,j,c,m], TensorFlow 'same' pads."""
    B, H, W, C = x.shape
    kh, kw, _, dm = w.shape
    if padding == "same":
        Ho, Wo = -(-H // sh), -(-W // sw)
        pt, pl = max((Ho - 1) * sh + kh - H, 0) // 2, max((Wo - 1) * sw + kw - W, 0) // 2
    else:
        Ho, Wo, pt, pl = (H - kh) // sh + 1, (W - kw) // sw + 1, 0, 0
    y = np.zeros((B, Ho, Wo, C * dm))
    for oh in range(Ho):
        for ow in range(Wo):
            for i in range(kh):
                for j in range(kw):
                    h, v = oh * sh - pt + i, ow * sw - pl + j
                    if 0 <= h < H and 0 <= v < W:
                        y[:, oh, ow] += (x[:, h, v, :, None] * w[i, j]).reshape(B, C * dm)
    return y


@pytest.mark.parametrize("B,H,W,C,dm,kh,kw,sh,sw,pad", CASES)
def test_ref_call_matches_nested_loops(B, H, W, C, dm, kh, kw, sh, sw, pad):
    rng = np.random.default_rng(0)
    x, w, pw = rng.standard_normal((B, H, W, C)), rng.standard_normal((kh, kw, C, dm)), rng.standard_normal((C * dm, 5))
    bias = rng.standard_normal(C * dm)
    want = _loops(x, w, sh, sw, pad)
    t = torch.from_numpy
    dwl = L.DepthwiseConv2D((kh, kw), strides=(sh, sw), padding=pad, depth_multiplier=dm)
    assert dwl._build_shapes((H, W, C)) == want.shape[1:]
    got = dwl.ref_call(t(x), {"depthwise_kernel": t(w), "bias": t(bias)}, False).numpy()
    assert np.abs(got - (want + bias)).max() / np.abs(want).max() < 1e-12
    sep = L.SeparableConv2D(5, (kh, kw), strides=(sh, sw), padding=pad, depth_multiplier=dm, activation="relu",
                            use_bias=False)
    assert sep._build_shapes((H, W, C)) == want.shape[1:3] + (5,)
    got = sep.ref_call(t(x), {"depthwise_kernel": t(w), "pointwise_kernel": t(pw)[None, None]}, False).numpy()
    ref = np.maximum(want @ pw, 0)
    assert np.abs(got - ref).max() / np.abs(ref).max() < 1e-12


def test_weights_counts_config_and_regularizers():
    inp = tde.keras.Input((12, 12, 3))
    d = L.DepthwiseConv2D(3, strides=2, padding="same", depth_multiplier=2, depthwise_regularizer=tde.regularizers.L2(0.1))
    s = L.SeparableConv2D(7, (3, 5), depth_multiplier=2, pointwise_regularizer=tde.regularizers.L1(0.2), name="sep")
    out = L.Dense(4)(L.GlobalAveragePooling2D()(s(d(inp))))
    m = tde.Model(inputs=inp, outputs=out)
    m.build()
    assert d.output_shape == (6, 6, 6) and s.output_shape == (4, 2, 7)
    assert [(w.name, w.shape) for w in d.weight_specs] == [("depthwise_kernel", (3, 3, 3, 2)), ("bias", (6,))]
    assert [(w.name, w.shape) for w in s.weight_specs] == [("depthwise_kernel", (3, 5, 6, 2)),
                                                           ("pointwise_kernel", (1, 1, 12, 7)), ("bias", (7,))]
    assert d.count_params() == 54 + 6 and s.count_params() == 180 + 84 + 7
    assert len(m.losses) == 2
    for lay in (d, s):
        cfg = lay.get_config()
        twin = L.from_config(type(lay).__name__, cfg)
        assert twin.get_config() == cfg and type(twin) is type(lay)
    assert not isinstance(d, L.Conv2D)   # the fused-plan matchers go by layer type


@pytest.mark.parametrize("cls,args", [(L.DepthwiseConv2D, (3,)), (L.SeparableConv2D, (8, 3))])
def test_dilation_and_data_format_are_refused(cls, args):
    with pytest.raises(ValueError, match="dilation"):
        cls(*args, dilation_rate=2)
    with pytest.raises(ValueError, match="channels_last"):
        cls(*args, data_format="channels_first")


def _compiled():
    tde.backend.set_random_seed(3)
    m = tde.zoo.mnist_separable_cnn()
    m.compile(loss=tde.losses.SparseCategoricalCrossentropy(from_logits=True), optimizer=tde.optimizers.SGD(0.05))
    return m


def test_zoo_model_trains_on_the_reference_plan():
    m = _compiled()
    assert m.count_params() == 3994 + 64
    rng = np.random.default_rng(1)
    x = rng.random((64, 28, 28, 1), dtype=np.float32)
    y = x.reshape(64, -1)[:, :10].argmax(1)
    h = m.fit(x, y, batch_size=16, epochs=4, verbose=0).history["loss"]
    assert h[-1] < h[0]


def test_saved_model_graph_reproduces_predict():
    from test_io import _decode_attr

    from tensorflow_distributed_example_amd.io import saved_model_pb as SM
    from tensorflow_distributed_example_amd.io import tf_proto
    m = _compiled()
    m.build()
    g, in_t, out_t, _, _ = SM.build_graph(m)
    gd = tf_proto.classes()["GraphDef"]()
    gd.ParseFromString(g.graph_def())
    nodes = [(n.name, n.op, list(n.input), {k: _decode_attr(v) for k, v in n.attr.items()}) for n in gd.node]
    assert [n[1] for n in nodes].count("DepthwiseConv2dNative") == 2
    x = np.random.default_rng(2).random((5, 28, 28, 1), dtype=np.float32)
    bundle = {n: m._store.view(n).numpy() for n in m._store.order}
    got = SM.run_graph(nodes, {in_t.split(":")[0]: x}, bundle, out_t)
    want = m.predict(x, verbose=0)
    assert np.allclose(got, want, rtol=1e-4, atol=1e-5), np.abs(got - want).max()

"""RandomRotation / RandomZoom on the host: the layers, their placement, the header's sine and cosine, the numpy
twin (ops/augment.py) against the float64 oracle (tests/augment_affine_oracle.py), and the reference-plan fit.

Bounds.  u = 2^-24 bounds the relative error of one rounded f32 operation.

Sine and cosine.  SINCOS_MEASURED is the largest |c - cos(2 pi f)|, |s - sin(2 pi f)| over all 2^24 draws of the
range [-1, 1] (the sweep below prints it; profiles/augment_affine/NOTES.md records it); SINCOS_BOUND is twice
that.  The norm: c^2 + s^2 - 1 = 2 (c dc + s ds) + dc^2 + ds^2 with |dc|, |ds| <= SINCOS_BOUND and
|c| + |s| <= sqrt 2 gives |c^2 + s^2 - 1| <= 2 sqrt 2 SINCOS_BOUND + 2 SINCOS_BOUND^2 (NORM_BOUND).  SINCOS_BOUND
itself cannot bound the norm of any f32 pair: cos and sin correctly rounded to f32 err by 2.98e-8 at most and
still reach |c^2 + s^2 - 1| = 8.39e-8 = 2.8 times that over the same sweep (measured; here 2.11e-7 = 2.39 times).

Source coordinates.  With ext = max(H, W): |vy|, |vx| < ext / 2, so the error of c and s moves a coordinate by at
most SINCOS_BOUND ext; the two products (<= ext / 2 each), their sum (<= ext), the centre's addition (<= 1.5 ext),
the addition of 0.5 or the subtraction of the floor (<= 1.5 ext + 1) round by at most 6 u ext together.  A zoom
has exact inputs (zh, zw are the twin's) and fewer operations.  COORD(ext) = (SINCOS_BOUND + 6 u) ext.

Bilinear.  The interpolant of the filled image is continuous and changes by at most D per unit of a coordinate,
D <= 2 M the largest step between neighbours, M = max(|x|, |fill_value|): two coordinates within COORD move it by
4 M COORD; the four f32 weights, products and three adds round by 6 u M (tests/test_augment.py's bilinear bound).
Nearest.  Equal to the oracle except where a float64 coordinate lies within COORD of a half-integer tie; at most
2 % of a case's pixels may be left out for that, and the seeds are chosen so that they are.
"""
import ctypes
import json

import numpy as np
import pytest

import augment_affine_oracle as FO
import tensorflow_distributed_example_amd as tde
from tensorflow_distributed_example_amd.models import zoo
from tensorflow_distributed_example_amd.ops import augment as AU

L = tde.keras.layers
U, SINCOS_MEASURED, SINCOS_BOUND = FO.U, FO.SINCOS_MEASURED, FO.SINCOS_BOUND
NORM_BOUND = 2 * np.sqrt(2.0) * SINCOS_BOUND + 2 * SINCOS_BOUND ** 2
coord_bound, bilinear_bound = FO.coord_bound, FO.bilinear_bound
SHAPES = [(1, 1, 1), (5, 7, 1), (4, 4, 3), (8, 8, 4), (28, 28, 1)]
FILLS = L.RandomRotation.FILL_MODES
INTERPS = L.RandomRotation.INTERPOLATIONS
FILL = 0.125


def _ids(s):
    return "x".join(map(str, s))


# ------------------------------------------------------------------------------------ the layers
def test_constructor_rules():
    r = L.RandomRotation(0.25)
    assert r.factor_range == (-0.25, 0.25)
    assert (r.fill_mode, r.interpolation, r.fill_value, r.seed) == ("reflect", "bilinear", 0.0, None)
    assert L.RandomRotation((-0.5, 0.1)).factor_range == (-0.5, 0.1)
    assert L.RandomRotation(1).factor_range == (-1.0, 1.0)
    z = L.RandomZoom(0.25)
    assert z.height_range == (-0.25, 0.25) and z.width_range is None and z.width_factor is None
    assert (z.fill_mode, z.interpolation, z.fill_value, z.seed) == ("reflect", "bilinear", 0.0, None)
    assert L.RandomZoom(0.25, (-0.5, 0.1)).width_range == (-0.5, 0.1)
    for bad in (-0.1, (0.2, 0.1), (-1.5, 0.0), (0.0, 1.5), (0.1,), "0.1", None, 1.5, True):
        with pytest.raises(ValueError, match="RandomRotation: factor"):
            L.RandomRotation(bad)
        with pytest.raises(ValueError, match="RandomZoom: height_factor"):
            L.RandomZoom(bad)
        if bad is not None:
            with pytest.raises(ValueError, match="RandomZoom: width_factor"):
                L.RandomZoom(0.1, bad)
    with pytest.raises(ValueError, match="must not be negative"):
        L.RandomRotation(-0.1)
    with pytest.raises(ValueError, match="needs -1 <= lo <= hi <= 1"):
        L.RandomZoom((0.2, 0.1))
    for cls, args in ((L.RandomRotation, (0.1,)), (L.RandomZoom, (0.1,))):
        with pytest.raises(ValueError, match=f"{cls.__name__}: fill_mode"):
            cls(*args, fill_mode="mirror")
        with pytest.raises(ValueError, match=f"{cls.__name__}: interpolation"):
            cls(*args, interpolation="bicubic")
    with pytest.raises(ValueError):   # rank-3 channels_last inputs only
        tde.keras.Sequential([L.RandomRotation(0.1, input_shape=(784,)), L.Dense(10)])
    assert issubclass(L.RandomRotation, L.InputStageLayer) and issubclass(L.RandomZoom, L.InputStageLayer)
    assert L.LAYER_CLASSES["RandomRotation"] is L.RandomRotation and L.LAYER_CLASSES["RandomZoom"] is L.RandomZoom


def _stage():
    return [L.RandomRotation(0.05, seed=3), L.RandomZoom(0.1, interpolation="nearest")]


def test_config_round_trip_and_summary():
    m = zoo.with_input_stage(zoo.lenet5(), [L.RandomRotation((-0.5, 0.1), fill_mode="wrap", interpolation="nearest",
                                                             seed=7, fill_value=0.5),
                                            L.RandomZoom(0.25, (-0.1, 0.2), fill_mode="constant", seed=3),
                                            L.RandomZoom((-0.3, 0.0), interpolation="nearest")])
    m2 = tde.keras.Sequential.from_config(json.loads(m.to_json())["config"])
    assert json.loads(json.dumps(m2.get_config())) == json.loads(json.dumps(m.get_config()))
    a, b, c = m2.input_stage
    assert (type(a), a.factor_range, a.fill_mode, a.interpolation, a.seed, a.fill_value) == \
        (L.RandomRotation, (-0.5, 0.1), "wrap", "nearest", 7, 0.5)
    assert (type(b), b.height_range, b.width_range, b.fill_mode, b.interpolation, b.seed) == \
        (L.RandomZoom, (-0.25, 0.25), (-0.1, 0.2), "constant", "bilinear", 3)
    assert (c.height_range, c.width_range, c.seed) == ((-0.3, 0.0), None, None)
    for l in m.input_stage:
        r = L.from_config(type(l).__name__, l.get_config())
        assert type(r) is type(l) and r.get_config() == l.get_config()
        assert l.count_params() == 0 and l.weight_specs == [] and l.output_shape == (28, 28, 1)
    lines = []
    m.summary(print_fn=lines.append)
    rows = [ln for ln in lines if "Random" in ln]
    assert len(rows) == 3 and all(ln.split()[-1] == "0" for ln in rows)
    assert sum("random_rotation" in ln for ln in rows) == 1 and sum("random_zoom" in ln for ln in rows) == 2
    assert m.count_params() == zoo.lenet5().count_params()
    # the ctypes layers: the new kinds in the existing fields
    la, lb, lc = (l.aug_layer(j) for j, l in enumerate(m.input_stage))
    assert (la.kind, la.mode, la.bilinear, la.j, la.seed, la.pad_) == (AU.ROTATE, 3, 0, 0, 7, 0)
    assert (la.lo_h, la.hi_h, la.fill_value) == (-0.5, np.float32(0.1), 0.5)
    assert (lb.kind, lb.mode, lb.bilinear, lb.j, lb.pad_) == (AU.ZOOM, 0, 1, 1, 0)
    assert (lb.lo_h, lb.hi_h, lb.lo_w, lb.hi_w) == (-0.25, 0.25, np.float32(-0.1), np.float32(0.2))
    assert (lc.kind, lc.bilinear, lc.j, lc.pad_, lc.lo_w, lc.hi_w) == (AU.ZOOM, 0, 2, 1, 0.0, 0.0)


def test_checkpoint_and_export_equal_the_plain_models(tmp_path):
    from tensorflow_distributed_example_amd.io import export as EX
    from tensorflow_distributed_example_amd.io import object_graph as OG
    from tensorflow_distributed_example_amd.io import tensor_bundle as TB
    plain = zoo.lenet5()
    aug = zoo.with_input_stage(plain, _stage())          # the same layer names
    for m in (plain, aug):
        m.compile("sgd", tde.keras.losses.SparseCategoricalCrossentropy(from_logits=True), metrics=["accuracy"])
    aug.set_weights(plain.get_weights())
    assert list(OG.variable_keys(aug).values()) == list(OG.variable_keys(plain).values())
    assert [type(l).__name__ for l, _, _ in aug._nodes()] == [type(l).__name__ for l, _, _ in plain._nodes()]
    values = {n: v.numpy() for n, v in plain.state_dict().items()}
    ga, gp = OG.build(aug, values, iterations=3), OG.build(plain, values, iterations=3)
    assert list(ga) == list(gp)
    for k in gp:
        a, b = ga[k], gp[k]
        assert (a == b) if isinstance(b, bytes) else np.array_equal(a, b), k
    files = {}
    for tag, m in (("aug", aug), ("plain", plain)):
        m.save_weights(str(tmp_path / tag / "ckpt"))
        files[tag] = TB.read_bundle(str(tmp_path / tag / "ckpt"))
    assert list(files["aug"]) == list(files["plain"])
    for k, b in files["plain"].items():
        a = files["aug"][k]
        assert (a == b) if isinstance(b, (bytes, str)) else np.array_equal(a, b), k
    fresh = zoo.with_input_stage(zoo.lenet5(), _stage())
    fresh.compile("sgd", tde.keras.losses.SparseCategoricalCrossentropy(from_logits=True))
    fresh.load_weights(str(tmp_path / "plain" / "ckpt"))          # and the plain model's checkpoint loads
    for a, b in zip(fresh.get_weights(), plain.get_weights()):
        assert np.array_equal(a, b)
    pbs = {}
    for tag, m in (("aug", aug), ("plain", plain)):
        out = EX.export_saved_model(m, str(tmp_path / tag / "export"), None).decode()
        pbs[tag] = open(out + "/saved_model.pb", "rb").read()
        assert sorted(TB.read_bundle(out + "/variables/variables")) == sorted(m.state_dict())
    assert pbs["aug"] == pbs["plain"] and len(pbs["plain"]) > 0


def test_identity_outside_training():
    rng = np.random.default_rng(0)
    x = rng.standard_normal((20, 28, 28, 1)).astype(np.float32)
    y = rng.integers(0, 10, 20)
    plain = zoo.lenet5()
    aug = zoo.with_input_stage(zoo.lenet5(), _stage())
    for m in (plain, aug):
        m.compile("sgd", "sparse_categorical_crossentropy", metrics=["accuracy"])
    aug.set_weights(plain.get_weights())
    assert np.array_equal(aug.predict(x, batch_size=8), plain.predict(x, batch_size=8))
    assert aug.evaluate(x, y, batch_size=8, verbose=0) == plain.evaluate(x, y, batch_size=8, verbose=0)
    assert np.array_equal(aug(x).cpu().numpy(), plain(x).cpu().numpy())


def _compile(stage):
    zoo.with_input_stage(zoo.mnist_mlp(), stage).compile("sgd", "sparse_categorical_crossentropy")


def test_placement_and_composition_refusals():
    for late in (L.RandomRotation(0.1, name="late_turn"), L.RandomZoom(0.1, name="late_zoom")):
        m = tde.keras.Sequential([L.Conv2D(4, 3, activation="relu", input_shape=(8, 8, 1)), late, L.Flatten(),
                                  L.Dense(3)])
        with pytest.raises(ValueError, match=late.name):
            m.compile("sgd", "sparse_categorical_crossentropy")
    inp = L.Input((8, 8, 1))
    a = L.RandomZoom(0.1, name="forked_zoom")(inp)     # the input has two consumers: no input stage
    out = L.Dense(3)(L.Flatten()(L.Add()([a, L.Conv2D(1, 1)(inp)])))
    with pytest.raises(ValueError, match="forked_zoom"):
        tde.keras.Model(inp, out).compile("sgd", "sparse_categorical_crossentropy")
    with pytest.raises(ValueError, match="at most 4"):
        _compile([L.RandomRotation(0.1, interpolation="nearest") for _ in range(5)])
    with pytest.raises(ValueError) as e:
        _compile([L.RandomRotation(0.1, name="turn_a"), L.RandomFlip(), L.RandomZoom(0.1, name="zoom_b")])
    msg = str(e.value)
    assert "turn_a" in msg and "zoom_b" in msg and "RandomRotation" in msg and "RandomZoom" in msg
    assert "interpolation='nearest'" in msg and "chain freely" in msg
    with pytest.raises(ValueError, match="turn_a.*move_b"):
        _compile([L.RandomRotation(0.1, name="turn_a"), L.RandomTranslation(0.1, 0.1, name="move_b")])
    with pytest.raises(ValueError, match="zoom_a.*zoom_b"):
        _compile([L.RandomZoom(0.1, name="zoom_a"), L.RandomZoom(0.1, name="zoom_b")])
    # two bilinear translations: the message of before
    with pytest.raises(ValueError, match="at most one RandomTranslation with interpolation='bilinear'"):
        _compile([L.RandomTranslation(0.1, 0.1), L.RandomTranslation(0.1, 0.1)])
    # nearest layers chain freely around one interpolating layer
    _compile([L.RandomRotation(0.1, interpolation="nearest"), L.RandomZoom(0.1, interpolation="nearest"),
              L.RandomTranslation(0.1, 0.1)])
    _compile([L.RandomFlip(), L.RandomRotation(0.1, interpolation="nearest"), L.RandomZoom(0.1),
              L.RandomTranslation(0.1, 0.1, interpolation="nearest")])
    inp = L.Input((8, 8, 1))                       # the functional form of a well-placed stage
    out = L.Dense(3)(L.Flatten()(L.RandomZoom(0.1, interpolation="nearest")(L.RandomRotation(0.1)(inp))))
    fm = tde.keras.Model(inp, out)
    fm.compile("sgd", "sparse_categorical_crossentropy")
    assert [type(l).__name__ for l in fm.input_stage] == ["RandomRotation", "RandomZoom"]
    assert [(type(l).__name__, ins, o) for l, ins, o in fm._nodes()] == [("Flatten", [0], 1), ("Dense", [1], 2)]


def test_struct_sizes_unchanged():
    assert ctypes.sizeof(AU.AugLayer) == 48 and ctypes.sizeof(AU.AugSpec) == 8 + 4 * 48
    assert [n for n, _ in AU.AugLayer._fields_] == ["kind", "mode", "bilinear", "j", "seed", "lo_h", "hi_h", "lo_w",
                                                     "hi_w", "fill_value", "pad_"]


# ------------------------------------------------------------------------------------ sine and cosine
@pytest.fixture(scope="module")
def sweep():
    """c, s of every one of the 2^24 draws of the range [-1, 1], and their float64 references."""
    u = np.arange(2 ** 24, dtype=np.uint32).astype(np.float32) * np.float32(2.0 ** -24)
    f = AU._draw1(-1.0, 1.0, u)
    c, s = AU.sincos(f)
    a = 2.0 * np.pi * f.astype(np.float64)
    return f, c, s, np.cos(a), np.sin(a)


def test_sincos_sweep_against_float64(sweep):
    f, c, s, c64, s64 = sweep
    assert c.dtype == np.float32 and s.dtype == np.float32 and len(np.unique(f)) == 2 ** 24
    ec, es = float(np.abs(c - c64).max()), float(np.abs(s - s64).max())
    print(f"sincos over 2^24 draws of [-1, 1]: max |c - cos| {ec:.4g}, max |s - sin| {es:.4g}, "
          f"bound {SINCOS_BOUND:.4g} (measured {SINCOS_MEASURED:.4g})")
    assert max(ec, es) <= SINCOS_BOUND
    assert max(ec, es) >= SINCOS_MEASURED / 2          # and the recorded figure is this code's


def test_sincos_quarter_turns_exact():
    want = {0: (1, 0), 1: (0, 1), 2: (-1, 0), 3: (0, -1)}
    for q in range(-4, 5):
        c, s = AU.sincos(np.float32(q / 4.0))
        assert (float(c), float(s)) == want[q % 4], q
    # through the draw: lo = hi, and the ends of [-1, 1]
    for lo, hi, u, q in ((0.25, 0.25, 0.7, 1), (-0.75, -0.75, 0.3, 1), (-1.0, 1.0, 0.0, 0), (-1.0, 1.0, 0.5, 0),
                         (-1.0, 1.0, 0.625, 1), (-1.0, 1.0, 0.25, 2)):
        c, s = AU.sincos(AU._draw1(lo, hi, np.float32(u)))
        assert (float(c), float(s)) == want[q], (lo, hi, u)


def test_sincos_norm(sweep):
    _, c, s, _, _ = sweep
    n = float(np.abs(c.astype(np.float64) ** 2 + s.astype(np.float64) ** 2 - 1.0).max())
    print(f"max |c^2 + s^2 - 1| {n:.4g}, bound {NORM_BOUND:.4g}")
    assert n <= NORM_BOUND


# ------------------------------------------------------------------------------------ exact cases
def _one(layer, x, B=3, t=5):
    return AU.apply(AU.stage_spec([layer]), x, B, t)


def _images(shape, n=4, seed=1):
    x = np.random.default_rng(seed).standard_normal((n,) + shape).astype(np.float32)
    x.reshape(-1)[::5] = -0.0
    return x


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@pytest.mark.parametrize("ip", INTERPS)
@pytest.mark.parametrize("fm", FILLS)
def test_right_angles_and_identities_exact(fm, ip):
    kw = dict(fill_mode=fm, interpolation=ip, seed=4, fill_value=FILL)
    for shape in ((4, 4, 3), (8, 8, 4), (7, 7, 1), (28, 28, 1), (1, 1, 1)):
        x = _images(shape)
        got = _one(L.RandomRotation((0.25, 0.25), **kw), x)
        assert np.array_equal(_bits(got), _bits(np.stack([np.rot90(im, 1) for im in x]))), shape
        got = _one(L.RandomRotation((-0.25, -0.25), **kw), x)
        assert np.array_equal(_bits(got), _bits(np.stack([np.rot90(im, -1) for im in x]))), shape
    for shape in SHAPES + [(6, 3, 2)]:
        x = _images(shape)
        for f in (0.5, -0.5):
            assert np.array_equal(_bits(_one(L.RandomRotation((f, f), **kw), x)), _bits(x[:, ::-1, ::-1])), shape
        for ident in (L.RandomRotation(0, **kw), L.RandomRotation((1.0, 1.0), **kw), L.RandomZoom(0, **kw),
                      L.RandomZoom(0, 0, **kw)):
            assert np.array_equal(_bits(_one(ident, x)), _bits(x)), (shape, type(ident).__name__)


@pytest.mark.parametrize("fm", FILLS)
def test_hand_computed_zoom_nearest(fm):
    """4 x 4, cy = 1.5.  Factor 1 (z = 2): s = 1.5 + 2 (i - 1.5) = -1.5, 0.5, 2.5, 4.5, nearest floor(s + 0.5) = -1,
    1, 3, 5.  Factor -0.5 (z = 0.5): s = 0.75, 1.25, 1.75, 2.25, nearest 1, 1, 2, 2."""
    x = np.arange(16, dtype=np.float32).reshape(1, 4, 4, 1) + 1
    outside = {"constant": (None, None), "nearest": (0, 3), "reflect": (0, 2), "wrap": (3, 1)}[fm]   # of -1 and 5
    idx = [outside[0], 1, 3, outside[1]]
    want = np.full((4, 4), FILL, np.float32)
    for y in range(4):
        for xx in range(4):
            if idx[y] is not None and idx[xx] is not None:
                want[y, xx] = x[0, idx[y], idx[xx], 0]
    got = _one(L.RandomZoom((1.0, 1.0), fill_mode=fm, interpolation="nearest", fill_value=FILL), x)
    assert np.array_equal(got[0, :, :, 0], want)
    got = _one(L.RandomZoom((-0.5, -0.5), fill_mode=fm, interpolation="nearest", fill_value=FILL), x)
    assert np.array_equal(got[0, :, :, 0], x[0, :, :, 0][[1, 1, 2, 2]][:, [1, 1, 2, 2]])
    # the axes on their own: height out, width in
    got = _one(L.RandomZoom((1.0, 1.0), (-0.5, -0.5), fill_mode=fm, interpolation="nearest", fill_value=FILL), x)
    ref = np.full((4, 4), FILL, np.float32)
    for y in range(4):
        if idx[y] is not None:
            ref[y] = x[0, idx[y], :, 0][[1, 1, 2, 2]]
    assert np.array_equal(got[0, :, :, 0], ref)


# ------------------------------------------------------------------------------------ the twin against float64
def _cases():
    """(tag, layer factory(fill_mode, interpolation), rotation?)"""
    return [("turn_0.15", lambda **kw: L.RandomRotation(0.15, seed=4, **kw), True),
            ("turn_full", lambda **kw: L.RandomRotation((-1.0, 1.0), seed=12, **kw), True),
            ("zoom_same", lambda **kw: L.RandomZoom((-0.5, 0.7), seed=6, **kw), False),
            ("zoom_both", lambda **kw: L.RandomZoom((-0.9, 0.3), (-0.2, 1.0), seed=8, **kw), False)]


def _draw_dicts(spec, stage, t, rows, H, W):
    """Per row, the oracle's draws of every layer: the twin's drawn values."""
    per = [AU.layer_rows(spec.layer[k], t, rows, H, W) for k in range(spec.n)]
    keys = {"RandomFlip": ("hflip", "vflip"), "RandomTranslation": ("dy", "dx"), "RandomRotation": ("f",),
            "RandomZoom": ("zh", "zw")}
    return [[{k: d[k][r] for k in keys[type(l).__name__]} for l, d in zip(stage, per)] for r in range(rows)]


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_twin_bilinear_within_bound(shape):
    H, W, _ = shape
    x = _images(shape, n=3, seed=2)
    M = max(float(np.abs(x).max()), FILL)
    worst = 0.0
    for tag, make, rot in _cases():
        bound = bilinear_bound(max(H, W), M, rot)
        for fm in FILLS:
            stage = [make(fill_mode=fm, interpolation="bilinear", fill_value=FILL)]
            spec = AU.stage_spec(stage)
            got = AU.apply(spec, x, 3, 5)
            dr = _draw_dicts(spec, stage, 5, 3, H, W)
            for r in range(3):
                want = FO.transform(x[r], [FO.layer_of(l) for l in stage], dr[r])
                err = float(np.abs(got[r].astype(np.float64) - want).max())
                worst = max(worst, err / bound)
                assert err <= bound, (tag, fm, r, err, bound)
    print(f"{shape}: worst bilinear error / bound {worst:.3g}")


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_twin_nearest_equal_off_the_ties(shape):
    H, W, _ = shape
    x = _images(shape, n=3, seed=3)
    for tag, make, rot in _cases():
        delta = coord_bound(max(H, W), rot)
        for fm in FILLS:
            stage = [make(fill_mode=fm, interpolation="nearest", fill_value=FILL)]
            spec = AU.stage_spec(stage)
            got = AU.apply(spec, x, 3, 5)
            dr = _draw_dicts(spec, stage, 5, 3, H, W)
            ol = [FO.layer_of(l) for l in stage]
            skipped = 0
            for r in range(3):
                want = FO.transform(x[r], ol, dr[r])
                tie = FO.near_tie(*FO.coords(ol[0], dr[r][0], H, W), delta)
                skipped += int(tie.sum())
                assert np.array_equal(got[r].astype(np.float64)[~tie], want[~tie]), (tag, fm, r)
            assert skipped <= 0.02 * 3 * H * W, (tag, fm, skipped)     # the cap: on the oracle's coordinates alone


def test_twin_composed_stage_against_oracle():
    """Flip + nearest rotation + bilinear zoom + nearest translation: the walk through every kind."""
    shape = (8, 8, 4)
    H, W, _ = shape
    x = _images(shape, n=5, seed=4)
    stage = [L.RandomFlip(seed=2), L.RandomRotation(0.2, fill_mode="wrap", interpolation="nearest", seed=3),
             L.RandomZoom(0.3, fill_mode="constant", seed=5, fill_value=FILL),
             L.RandomTranslation(0.2, 0.2, fill_mode="reflect", interpolation="nearest", seed=7)]
    spec = AU.stage_spec(stage)
    got = AU.apply(spec, x, 2, 9)
    ol = [FO.layer_of(l) for l in stage]
    bound = bilinear_bound(8, max(float(np.abs(x).max()), FILL), False)
    moved = 0
    for i in range(5):
        dr = _draw_dicts(spec, stage, 9 + i // 2, 2, H, W)[i % 2]
        tie = FO.near_tie(*FO.coords(ol[1], dr[1], H, W), coord_bound(8))
        if tie.any():     # a tie of the rotation in front moves a whole neighbour: not this test's subject
            continue
        want = FO.transform(x[i], ol, dr)
        assert float(np.abs(got[i].astype(np.float64) - want).max()) <= bound, i
        moved += 1
    assert moved >= 3


def test_width_follows_the_height_draw():
    lay = L.RandomZoom(0.4, seed=5).aug_layer(0)
    d = AU.layer_rows(lay, 3, 64, 28, 28)
    assert np.array_equal(d["zh"], d["zw"]) and len(np.unique(d["zh"])) > 32
    assert (d["zh"] >= np.float32(0.6)).all() and (d["zh"] <= np.float32(1.4)).all()
    both = L.RandomZoom(0.4, 0.4, seed=5).aug_layer(0)
    e = AU.layer_rows(both, 3, 64, 28, 28)
    assert np.array_equal(e["zh"], d["zh"]) and not np.array_equal(e["zw"], e["zh"])     # u2 the height, u3 the width
    # the rotation draws from u0
    u = AU.units(9, 3, 1, 16)
    r = AU.layer_rows(L.RandomRotation((-0.5, 0.25), seed=9).aug_layer(1), 3, 16, 28, 28)
    assert np.array_equal(r["f"], AU._draw1(-0.5, 0.25, u[:, 0]))
    p = AU.row_params(AU.stage_spec([L.RandomFlip(seed=1), L.RandomZoom(0.4, seed=5)]), 3, 8, 28, 28)
    assert p.shape == (8, 16) and not p[:, 8:].any() and np.array_equal(p[:, 4], p[:, 5])
    assert set(np.unique(p[:, :2])) <= {0.0, 1.0}


# ------------------------------------------------------------------------------------ the reference-plan fit
@pytest.mark.parametrize("spe", [1, 4])
def test_reference_fit_equals_fit_on_pretransformed_data(spe):
    rng = np.random.default_rng(3)
    n, batch, epochs = 34, 4, 2            # 8 full steps and a ragged batch of 2 per epoch
    x = rng.standard_normal((n, 8, 8, 1)).astype(np.float32)
    y = rng.integers(0, 3, n)

    def body():
        return tde.keras.Sequential([L.Conv2D(4, 3, activation="relu", input_shape=(8, 8, 1)), L.MaxPooling2D(),
                                     L.Flatten(), L.Dense(3)])

    stage = [L.RandomRotation(0.1, seed=21), L.RandomZoom(0.2, interpolation="nearest")]
    aug = zoo.with_input_stage(body(), stage)
    plain = body()
    for m in (aug, plain):
        m.compile(tde.keras.optimizers.SGD(0.05), "sparse_categorical_crossentropy", metrics=["accuracy"],
                  steps_per_execution=spe)
    plain.set_weights(aug.get_weights())
    w0 = [w.copy() for w in aug.get_weights()]
    h = aug.fit(x, y, batch_size=batch, epochs=epochs, shuffle=False, verbose=0)
    assert aug._programs and all(p.plan_kind == "reference" and p.aug is not None for p in aug._programs.values())
    assert aug.optimizer.iterations == 18
    spec = AU.stage_spec(aug.input_stage)
    losses, t = [], 0
    for e in range(epochs):
        xs = []
        for lo in range(0, n, batch):
            xb = x[lo: lo + batch]
            xs.append(AU.apply(spec, xb, len(xb), t))
            t += 1
        if e == 0:
            assert not np.array_equal(xs[0], x[:batch])   # the stage did move pixels
        losses += plain.fit(np.concatenate(xs), y, batch_size=batch, epochs=1, shuffle=False, verbose=0).history["loss"]
    assert any(not np.array_equal(a, b) for a, b in zip(w0, aug.get_weights()))
    for a, b in zip(aug.get_weights(), plain.get_weights()):
        assert np.array_equal(a, b)
    assert h.history["loss"] == losses

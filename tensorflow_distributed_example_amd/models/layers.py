"""Keras-compatible layers (channels_last / NHWC activations, HWIO conv kernels,
[in, out] dense kernels — byte-compatible with Keras/TF checkpoints).

Layers used by the reference models:
  * Model A (distributed_with_keras.py:33-39, tf2_mnist_distributed.py:66-72):
    Conv2D(32,3,relu) · MaxPooling2D · Flatten · Dense(64,relu) · Dense(10)
  * Model B (mnist_keras_distributed.py:79-109, tf2_mnist_distributed.py:105-135):
    Reshape · Conv2D(same, no bias) · BatchNormalization(scale=False) ·
    Activation('relu') · ... · Dropout(0.5) · Dense(10, softmax)
plus ResNet building blocks (ZeroPadding2D, GlobalAveragePooling2D, Add) for the
ResNet-18 stress config.

Each layer declares its weights (``WeightSpec``) and a reference forward made of
plain torch ops (``ref_call``) — the CPU backend's kernel library and the
numerics oracle for the HIP kernels.  On the GPU the training program replaces
layer chains by fused HIP stages (train/program.py).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Callable, Optional

import numpy as np
import torch
import torch.nn.functional as F

from .. import backend as K
from .. import regularizers
from . import initializers


@dataclass
class WeightSpec:
    name: str            # short name: "kernel", "bias", "beta", "moving_mean", ...
    shape: tuple
    initializer: Callable
    trainable: bool = True
    aggregation: str = "none"   # SyncOnRead aggregation for non-trainables ("mean")
    layer: "Layer" = field(default=None, repr=False)
    l1: float = 0.0      # regularizer coefficients (regularizers.py); both zero: none
    l2: float = 0.0

    @property
    def full_name(self):
        return f"{self.layer.name}/{self.name}"


def _reg_config(layer, *names):
    """The regularizers a layer has, serialized (``regularizers.get`` takes the form back); none: no key, so
    the config of an unregularized layer is what it always was."""
    return {n: regularizers.serialize(getattr(layer, n)) for n in names if getattr(layer, n) is not None}


def _tuple2(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def get_activation(a):
    if a is None or a == "linear":
        return None
    if callable(a):
        return a
    if a not in ("relu", "softmax", "sigmoid", "tanh"):
        raise ValueError(f"unsupported activation {a!r}")
    return a


def apply_activation(x, act):
    if act is None:
        return x
    if act == "relu":
        return F.relu(x)
    if act == "softmax":
        return torch.softmax(x, dim=-1)
    if act == "sigmoid":
        return torch.sigmoid(x)
    if act == "tanh":
        return torch.tanh(x)
    return act(x)


def tf_same_pads(n, k, s):
    """TF 'SAME' padding: pad_total = max((ceil(n/s)-1)*s + k - n, 0); before = total//2."""
    out = -(-n // s)
    total = max((out - 1) * s + k - n, 0)
    return total // 2, total - total // 2


class KerasTensor:
    """Symbolic tensor of the functional API: a shape plus the layer call that produces it."""

    def __init__(self, shape, producer=None, inputs=(), name=None):
        self.shape = (None,) + tuple(int(d) for d in shape)
        self.producer = producer
        self.inputs = list(inputs)
        self.name = name

    def __repr__(self):
        who = self.producer.name if self.producer is not None else self.name
        return f"<KerasTensor shape={self.shape} from {who}>"


def Input(shape=None, batch_size=None, name=None, dtype=None, batch_shape=None):
    """``keras.Input``: the symbolic model input (channels_last image or feature vector)."""
    if shape is None and batch_shape is not None:
        shape = tuple(batch_shape[1:])
    return KerasTensor(tuple(shape), name=name or K.unique_name("input"))


class Layer:
    _prefix = "layer"
    multi_input = False

    def __init__(self, name: Optional[str] = None, input_shape=None, trainable=True, **kwargs):
        for k in kwargs:
            if k == "activity_regularizer":
                if kwargs[k] is None:
                    continue
                raise TypeError(f"{type(self).__name__}: activity_regularizer is not supported (weight regularizers "
                                "are: kernel_regularizer / bias_regularizer, gamma_regularizer / beta_regularizer)")
            if k not in ("dtype", "batch_input_shape", "input_dim"):
                raise TypeError(f"{type(self).__name__}: unexpected argument {k!r}")
        if "input_dim" in kwargs and input_shape is None:
            input_shape = (kwargs["input_dim"],)
        self.name = name or K.unique_name(self._prefix)
        self.input_shape_arg = tuple(input_shape) if input_shape is not None else None
        self.trainable = trainable
        self.built = False
        self.weight_specs: list[WeightSpec] = []
        self.input_shape = None
        self.output_shape = None
        self._model = None  # owning model (weights live in its ParamStore)

    # ---- building
    def add_weight(self, name, shape, initializer="zeros", trainable=True, aggregation="none", regularizer=None):
        reg = regularizers.get(regularizer)
        l1, l2 = reg.coefficients if reg is not None else (0.0, 0.0)
        spec = WeightSpec(name, tuple(int(s) for s in shape), initializers.get(initializer),
                          trainable and self.trainable, aggregation, self, l1, l2)
        self.weight_specs.append(spec)
        return spec

    def build(self, input_shape):
        self.built = True

    def compute_output_shape(self, input_shape):
        return input_shape

    def _build_shapes(self, input_shape):
        if self.multi_input:
            self.input_shape = [tuple(x) for x in input_shape]
            self.built = True
            self.output_shape = tuple(self.compute_output_shape(self.input_shape))
            return self.output_shape
        self.input_shape = tuple(input_shape)
        if not self.built:
            self.build(self.input_shape)
            self.built = True
        self.output_shape = tuple(self.compute_output_shape(self.input_shape))
        return self.output_shape

    # ---- functional API: calling a layer on symbolic tensors records a graph node
    def __call__(self, inputs, **kw):
        multi = isinstance(inputs, (list, tuple))
        ins = list(inputs) if multi else [inputs]
        if not all(isinstance(t, KerasTensor) for t in ins):
            raise TypeError(f"{self.name}: layers are called on symbolic tensors from Input(); "
                            "use model.predict()/model(x) for eager execution")
        shapes = [t.shape[1:] for t in ins]
        out = self._build_shapes(shapes if multi else shapes[0])
        return KerasTensor(out, producer=self, inputs=ins)

    # ---- weights (views into the owning model's ParamStore)
    def w(self, name):
        return self._model._store.view(f"{self.name}/{name}")

    @property
    def weights(self):
        return [self.w(s.name) for s in self.weight_specs]

    @property
    def trainable_weights(self):
        return [self.w(s.name) for s in self.weight_specs if s.trainable]

    def count_params(self):
        return int(sum(np.prod(s.shape) for s in self.weight_specs))

    # ---- reference forward (torch ops)
    def ref_call(self, x, W: dict, training: bool, rng=None, state_updates=None):
        raise NotImplementedError

    def get_config(self):
        return {"name": self.name}

    def __repr__(self):
        return f"<{type(self).__name__} {self.name}>"


class InputLayer(Layer):
    _prefix = "input"

    def ref_call(self, x, W, training, rng=None, state_updates=None):
        return x


class Conv2D(Layer):
    _prefix = "conv2d"

    def __init__(self, filters, kernel_size, strides=(1, 1), padding="valid", activation=None,
                 use_bias=True, kernel_initializer="glorot_uniform", bias_initializer="zeros",
                 data_format=None, dilation_rate=(1, 1), kernel_regularizer=None, bias_regularizer=None, **kw):
        super().__init__(**kw)
        self.kernel_regularizer = regularizers.get(kernel_regularizer)
        self.bias_regularizer = regularizers.get(bias_regularizer)
        if data_format not in (None, "channels_last"):
            raise ValueError("only channels_last is supported (Keras default)")
        if _tuple2(dilation_rate) != (1, 1):
            raise ValueError("dilation is not supported")
        self.filters = int(filters)
        self.kernel_size = _tuple2(kernel_size)
        self.strides = _tuple2(strides)
        self.padding = padding.lower()
        if self.padding not in ("valid", "same"):
            raise ValueError(padding)
        self.activation = get_activation(activation)
        self.use_bias = use_bias
        self.kernel_initializer = kernel_initializer
        self.bias_initializer = bias_initializer

    def build(self, input_shape):
        cin = input_shape[-1]
        kh, kw = self.kernel_size
        self.add_weight("kernel", (kh, kw, cin, self.filters), self.kernel_initializer,
                        regularizer=self.kernel_regularizer)
        if self.use_bias:
            self.add_weight("bias", (self.filters,), self.bias_initializer, regularizer=self.bias_regularizer)
        self.built = True

    def pads(self, input_shape):
        H, W = input_shape[0], input_shape[1]
        if self.padding == "valid":
            return (0, 0), (0, 0)
        return tf_same_pads(H, self.kernel_size[0], self.strides[0]), tf_same_pads(W, self.kernel_size[1], self.strides[1])

    def compute_output_shape(self, s):
        H, W = s[0], s[1]
        kh, kw = self.kernel_size
        sh, sw = self.strides
        if self.padding == "valid":
            Ho, Wo = (H - kh) // sh + 1, (W - kw) // sw + 1
        else:
            Ho, Wo = -(-H // sh), -(-W // sw)
        return (Ho, Wo, self.filters)

    def ref_call(self, x, W, training, rng=None, state_updates=None):
        (pt, pb), (pl, pr) = self.pads(x.shape[1:])
        xc = x.permute(0, 3, 1, 2)
        if pt or pb or pl or pr:
            xc = F.pad(xc, (pl, pr, pt, pb))
        k = W["kernel"].permute(3, 2, 0, 1)
        y = F.conv2d(xc, k, W.get("bias"), stride=self.strides)
        return apply_activation(y.permute(0, 2, 3, 1), self.activation)

    def get_config(self):
        return dict(name=self.name, filters=self.filters, kernel_size=self.kernel_size, strides=self.strides,
                    padding=self.padding, activation=self.activation, use_bias=self.use_bias,
                    **_reg_config(self, "kernel_regularizer", "bias_regularizer"))


def _depthwise_ref(x, kernel, strides, pads):
    """NHWC depthwise convolution of x with a Keras depthwise_kernel [KH, KW, C, dm] in torch ops: a grouped
    conv (groups = C) whose output channel c*dm + m is filter m of input channel c."""
    (pt, pb), (pl, pr) = pads
    kh, kw, C, dm = kernel.shape
    xc = x.permute(0, 3, 1, 2)
    if pt or pb or pl or pr:
        xc = F.pad(xc, (pl, pr, pt, pb))
    k = kernel.reshape(kh, kw, 1, C * dm).permute(3, 2, 0, 1)
    return F.conv2d(xc, k, stride=strides, groups=C).permute(0, 2, 3, 1)


class DepthwiseConv2D(Layer):
    """Keras ``DepthwiseConv2D``: every input channel convolved with its own ``depth_multiplier`` filters
    (weights ``depthwise_kernel`` [KH, KW, C, dm], ``bias`` [C*dm]).  On the GPU: csrc/kernels/depthwise.hip.
    Not a ``Conv2D`` subclass: the plan matchers tell the layers apart by type."""
    _prefix = "depthwise_conv2d"

    def __init__(self, kernel_size, strides=(1, 1), padding="valid", depth_multiplier=1, activation=None,
                 use_bias=True, depthwise_initializer="glorot_uniform", bias_initializer="zeros",
                 data_format=None, dilation_rate=(1, 1), depthwise_regularizer=None, bias_regularizer=None, **kw):
        super().__init__(**kw)
        if data_format not in (None, "channels_last"):
            raise ValueError("only channels_last is supported (Keras default)")
        if _tuple2(dilation_rate) != (1, 1):
            raise ValueError("dilation is not supported")
        self.kernel_size = _tuple2(kernel_size)
        self.strides = _tuple2(strides)
        self.padding = padding.lower()
        if self.padding not in ("valid", "same"):
            raise ValueError(padding)
        self.depth_multiplier = int(depth_multiplier)
        if self.depth_multiplier < 1:
            raise ValueError(f"depth_multiplier must be positive, got {depth_multiplier}")
        self.filters = None   # output channels: C * depth_multiplier, known at build
        self.activation = get_activation(activation)
        self.use_bias = use_bias
        self.depthwise_initializer = depthwise_initializer
        self.bias_initializer = bias_initializer
        self.depthwise_regularizer = regularizers.get(depthwise_regularizer)
        self.bias_regularizer = regularizers.get(bias_regularizer)

    pads = Conv2D.pads
    compute_output_shape = Conv2D.compute_output_shape

    def _add_depthwise(self, cin):
        kh, kw = self.kernel_size
        self.add_weight("depthwise_kernel", (kh, kw, cin, self.depth_multiplier), self.depthwise_initializer,
                        regularizer=self.depthwise_regularizer)

    def build(self, input_shape):
        self.filters = input_shape[-1] * self.depth_multiplier
        self._add_depthwise(input_shape[-1])
        if self.use_bias:
            self.add_weight("bias", (self.filters,), self.bias_initializer, regularizer=self.bias_regularizer)
        self.built = True

    def ref_call(self, x, W, training, rng=None, state_updates=None):
        y = _depthwise_ref(x, W["depthwise_kernel"], self.strides, self.pads(x.shape[1:]))
        if self.use_bias:
            y = y + W["bias"]
        return apply_activation(y, self.activation)

    def get_config(self):
        return dict(name=self.name, kernel_size=self.kernel_size, strides=self.strides, padding=self.padding,
                    depth_multiplier=self.depth_multiplier, activation=self.activation, use_bias=self.use_bias,
                    **_reg_config(self, "depthwise_regularizer", "bias_regularizer"))


class SeparableConv2D(DepthwiseConv2D):
    """Keras ``SeparableConv2D``: a depthwise convolution, then a 1x1 convolution to ``filters`` channels
    (weights ``depthwise_kernel``, ``pointwise_kernel`` [1, 1, C*dm, filters], ``bias`` [filters]); the bias
    and the activation come after the pointwise step only."""
    _prefix = "separable_conv2d"

    def __init__(self, filters, kernel_size, strides=(1, 1), padding="valid", depth_multiplier=1, activation=None,
                 use_bias=True, depthwise_initializer="glorot_uniform", pointwise_initializer="glorot_uniform",
                 bias_initializer="zeros", data_format=None, dilation_rate=(1, 1), depthwise_regularizer=None,
                 pointwise_regularizer=None, bias_regularizer=None, **kw):
        super().__init__(kernel_size, strides=strides, padding=padding, depth_multiplier=depth_multiplier,
                         activation=activation, use_bias=use_bias, depthwise_initializer=depthwise_initializer,
                         bias_initializer=bias_initializer, data_format=data_format, dilation_rate=dilation_rate,
                         depthwise_regularizer=depthwise_regularizer, bias_regularizer=bias_regularizer, **kw)
        self.filters = int(filters)
        self.pointwise_initializer = pointwise_initializer
        self.pointwise_regularizer = regularizers.get(pointwise_regularizer)

    def build(self, input_shape):
        cin = input_shape[-1]
        self._add_depthwise(cin)
        self.add_weight("pointwise_kernel", (1, 1, cin * self.depth_multiplier, self.filters),
                        self.pointwise_initializer, regularizer=self.pointwise_regularizer)
        if self.use_bias:
            self.add_weight("bias", (self.filters,), self.bias_initializer, regularizer=self.bias_regularizer)
        self.built = True

    def ref_call(self, x, W, training, rng=None, state_updates=None):
        y = _depthwise_ref(x, W["depthwise_kernel"], self.strides, self.pads(x.shape[1:]))
        y = y @ W["pointwise_kernel"][0, 0]
        if self.use_bias:
            y = y + W["bias"]
        return apply_activation(y, self.activation)

    def get_config(self):
        return dict(filters=self.filters, **super().get_config(),
                    **_reg_config(self, "pointwise_regularizer"))


class Dense(Layer):
    _prefix = "dense"

    def __init__(self, units, activation=None, use_bias=True, kernel_initializer="glorot_uniform",
                 bias_initializer="zeros", kernel_regularizer=None, bias_regularizer=None, **kw):
        super().__init__(**kw)
        self.kernel_regularizer = regularizers.get(kernel_regularizer)
        self.bias_regularizer = regularizers.get(bias_regularizer)
        self.units = int(units)
        self.activation = get_activation(activation)
        self.use_bias = use_bias
        self.kernel_initializer = kernel_initializer
        self.bias_initializer = bias_initializer

    def build(self, input_shape):
        self.add_weight("kernel", (input_shape[-1], self.units), self.kernel_initializer,
                        regularizer=self.kernel_regularizer)
        if self.use_bias:
            self.add_weight("bias", (self.units,), self.bias_initializer, regularizer=self.bias_regularizer)
        self.built = True

    def compute_output_shape(self, s):
        return tuple(s[:-1]) + (self.units,)

    def ref_call(self, x, W, training, rng=None, state_updates=None):
        y = x @ W["kernel"]
        if self.use_bias:
            y = y + W["bias"]
        return apply_activation(y, self.activation)

    def get_config(self):
        return dict(name=self.name, units=self.units, activation=self.activation, use_bias=self.use_bias,
                    **_reg_config(self, "kernel_regularizer", "bias_regularizer"))


class _Pooling2D(Layer):
    def __init__(self, pool_size=(2, 2), strides=None, padding="valid", **kw):
        super().__init__(**kw)
        self.pool_size = _tuple2(pool_size)
        self.strides = _tuple2(strides) if strides is not None else self.pool_size
        self.padding = padding.lower()

    def compute_output_shape(self, s):
        H, W, C = s
        ph, pw = self.pool_size
        sh, sw = self.strides
        if self.padding == "valid":
            return ((H - ph) // sh + 1, (W - pw) // sw + 1, C)
        return (-(-H // sh), -(-W // sw), C)

    def get_config(self):
        return dict(name=self.name, pool_size=self.pool_size, strides=self.strides, padding=self.padding)


class MaxPooling2D(_Pooling2D):
    _prefix = "max_pooling2d"

    def ref_call(self, x, W, training, rng=None, state_updates=None):
        xc = x.permute(0, 3, 1, 2)
        if self.padding == "same":
            (pt, pb) = tf_same_pads(x.shape[1], self.pool_size[0], self.strides[0])
            (pl, pr) = tf_same_pads(x.shape[2], self.pool_size[1], self.strides[1])
            xc = F.pad(xc, (pl, pr, pt, pb), value=float("-inf"))
        y = F.max_pool2d(xc, self.pool_size, self.strides)
        return y.permute(0, 2, 3, 1)


class AveragePooling2D(_Pooling2D):
    _prefix = "average_pooling2d"

    def ref_call(self, x, W, training, rng=None, state_updates=None):
        xc = x.permute(0, 3, 1, 2)
        if self.padding == "same":   # Keras: a window averages over its elements inside the image only
            (pt, pb) = tf_same_pads(x.shape[1], self.pool_size[0], self.strides[0])
            (pl, pr) = tf_same_pads(x.shape[2], self.pool_size[1], self.strides[1])
            ones = F.pad(torch.ones_like(xc[:1, :1]), (pl, pr, pt, pb))
            cnt = F.avg_pool2d(ones, self.pool_size, self.strides, divisor_override=1)
            y = F.avg_pool2d(F.pad(xc, (pl, pr, pt, pb)), self.pool_size, self.strides, divisor_override=1) / cnt
        else:
            y = F.avg_pool2d(xc, self.pool_size, self.strides)
        return y.permute(0, 2, 3, 1)


class GlobalAveragePooling2D(Layer):
    _prefix = "global_average_pooling2d"

    def compute_output_shape(self, s):
        return (s[-1],)

    def ref_call(self, x, W, training, rng=None, state_updates=None):
        return x.mean(dim=(1, 2))


class GlobalAveragePooling1D(Layer):
    """[N, T, C] -> [N, C]: the mean over the steps (``tde_gap32`` with HW = T on the GPU)."""
    _prefix = "global_average_pooling1d"

    def __init__(self, data_format=None, keepdims=False, **kw):
        super().__init__(**kw)
        if keepdims:
            raise NotImplementedError("GlobalAveragePooling1D: keepdims=True is not supported")
        if data_format not in (None, "channels_last"):
            raise NotImplementedError(f"GlobalAveragePooling1D: data_format={data_format!r} is not supported")

    def __call__(self, inputs, mask=None):
        if mask is not None:
            raise NotImplementedError(f"{self.name} (GlobalAveragePooling1D): mask= is not supported")
        return super().__call__(inputs)

    def compute_output_shape(self, s):
        if len(s) != 2:
            raise ValueError(f"{self.name}: input [N, T, C] expected, got {(None,) + tuple(s)}")
        return (s[-1],)

    def ref_call(self, x, W, training, rng=None, state_updates=None):
        return x.mean(dim=1)


class ZeroPadding2D(Layer):
    _prefix = "zero_padding2d"

    def __init__(self, padding=(1, 1), **kw):
        super().__init__(**kw)
        if isinstance(padding, int):
            padding = ((padding, padding), (padding, padding))
        elif isinstance(padding[0], int):
            padding = ((padding[0], padding[0]), (padding[1], padding[1]))
        self.padding = padding

    def compute_output_shape(self, s):
        (t, b), (l, r) = self.padding
        return (s[0] + t + b, s[1] + l + r, s[2])

    def ref_call(self, x, W, training, rng=None, state_updates=None):
        (t, b), (l, r) = self.padding
        return F.pad(x, (0, 0, l, r, t, b))

    def get_config(self):
        return dict(name=self.name, padding=self.padding)


class Flatten(Layer):
    _prefix = "flatten"

    def compute_output_shape(self, s):
        return (int(np.prod(s)),)

    def ref_call(self, x, W, training, rng=None, state_updates=None):
        return x.reshape(x.shape[0], -1)  # row-major over (H, W, C): Keras order


class Reshape(Layer):
    _prefix = "reshape"

    def __init__(self, target_shape, **kw):
        super().__init__(**kw)
        self.target_shape = tuple(target_shape)

    def compute_output_shape(self, s):
        if int(np.prod(s)) != int(np.prod(self.target_shape)):
            raise ValueError(f"cannot reshape {s} to {self.target_shape}")
        return self.target_shape

    def ref_call(self, x, W, training, rng=None, state_updates=None):
        return x.reshape((x.shape[0],) + self.target_shape)

    def get_config(self):
        return dict(name=self.name, target_shape=self.target_shape)


class Activation(Layer):
    _prefix = "activation"

    def __init__(self, activation, **kw):
        super().__init__(**kw)
        self.activation = get_activation(activation)

    def ref_call(self, x, W, training, rng=None, state_updates=None):
        return apply_activation(x, self.activation)

    def get_config(self):
        return dict(name=self.name, activation=self.activation)


class ReLU(Activation):
    _prefix = "re_lu"

    def __init__(self, **kw):
        super().__init__("relu", **kw)

    def get_config(self):
        return dict(name=self.name)


class Dropout(Layer):
    _prefix = "dropout"

    def __init__(self, rate, noise_shape=None, seed=None, **kw):
        super().__init__(**kw)
        self.rate = float(rate)
        self.seed = seed

    def ref_call(self, x, W, training, rng=None, state_updates=None):
        if not K.resolve_training(training) or self.rate == 0.0:
            return x
        keep = 1.0 - self.rate
        mask = torch.rand(x.shape, generator=rng, device="cpu" if rng is not None else x.device)
        mask = (mask.to(x.device) < keep).to(x.dtype)
        return x * mask / keep

    def get_config(self):
        return dict(name=self.name, rate=self.rate)


class BatchNormalization(Layer):
    _prefix = "batch_normalization"

    def __init__(self, axis=-1, momentum=0.99, epsilon=1e-3, center=True, scale=True,
                 beta_initializer="zeros", gamma_initializer="ones",
                 moving_mean_initializer="zeros", moving_variance_initializer="ones", beta_regularizer=None,
                 gamma_regularizer=None, **kw):
        super().__init__(**kw)
        self.beta_regularizer = regularizers.get(beta_regularizer)
        self.gamma_regularizer = regularizers.get(gamma_regularizer)
        if axis not in (-1,):
            raise ValueError("BatchNormalization: only axis=-1 (channels_last) is supported")
        self.momentum = float(momentum)
        self.epsilon = float(epsilon)
        self.center = center
        self.scale = scale
        self.inits = (beta_initializer, gamma_initializer, moving_mean_initializer, moving_variance_initializer)

    def build(self, input_shape):
        c = input_shape[-1]
        if self.scale:
            self.add_weight("gamma", (c,), self.inits[1], regularizer=self.gamma_regularizer)
        if self.center:
            self.add_weight("beta", (c,), self.inits[0], regularizer=self.beta_regularizer)
        self.add_weight("moving_mean", (c,), self.inits[2], trainable=False, aggregation="mean")
        self.add_weight("moving_variance", (c,), self.inits[3], trainable=False, aggregation="mean")
        self.built = True

    @property
    def fused(self):
        # TF/Keras uses the fused kernel (Bessel-corrected moving variance) for 4-D input.
        return self.input_shape is not None and len(self.input_shape) == 3

    def ref_call(self, x, W, training, rng=None, state_updates=None):
        axes = tuple(range(x.dim() - 1))
        gamma = W.get("gamma")
        beta = W.get("beta")
        if K.resolve_training(training):
            mean = x.mean(dim=axes)
            var = x.var(dim=axes, unbiased=False)
            if state_updates is not None:
                n = x.numel() // x.shape[-1]
                var_upd = var * (n / max(n - 1, 1)) if self.fused else var
                m = self.momentum
                state_updates.append((f"{self.name}/moving_mean", W["moving_mean"] * m + mean.detach() * (1 - m)))
                state_updates.append((f"{self.name}/moving_variance",
                                      W["moving_variance"] * m + var_upd.detach() * (1 - m)))
        else:
            mean, var = W["moving_mean"], W["moving_variance"]
        y = (x - mean) * torch.rsqrt(var + self.epsilon)
        if gamma is not None:
            y = y * gamma
        if beta is not None:
            y = y + beta
        return y

    def get_config(self):
        return dict(name=self.name, momentum=self.momentum, epsilon=self.epsilon, center=self.center,
                    scale=self.scale, **_reg_config(self, "beta_regularizer", "gamma_regularizer"))


class _GroupNormBase(Layer):
    """Batch-independent normalisation over groups of the last axis: y = (x - mean) * rsqrt(var + epsilon) * gamma
    + beta with the population statistics of each (sample, group).  No moving state; training and inference
    agree.  On the GPU: csrc/kernels/groupnorm.hip (float32 policy)."""

    def _init_norm(self, axis, epsilon, center, scale, beta_initializer, gamma_initializer, beta_regularizer,
                   gamma_regularizer):
        self.axis = axis
        self.epsilon = float(epsilon)
        self.center = center
        self.scale = scale
        self.inits = (beta_initializer, gamma_initializer)
        self.beta_regularizer = regularizers.get(beta_regularizer)
        self.gamma_regularizer = regularizers.get(gamma_regularizer)

    def _check_axis(self, input_shape):
        if self.axis not in (-1, len(input_shape)):
            raise ValueError(f"{type(self).__name__}: only the last axis (channels_last) is supported, got "
                             f"axis={self.axis!r}")

    def _add_affine(self, c):
        if self.scale:
            self.add_weight("gamma", (c,), self.inits[1], regularizer=self.gamma_regularizer)
        if self.center:
            self.add_weight("beta", (c,), self.inits[0], regularizer=self.beta_regularizer)

    def _norm_config(self):
        return dict(name=self.name, axis=self.axis, epsilon=self.epsilon, center=self.center, scale=self.scale,
                    **_reg_config(self, "beta_regularizer", "gamma_regularizer"))


class GroupNormalization(_GroupNormBase):
    """Keras ``GroupNormalization`` on [N, H, W, C] and [N, C] inputs: statistics over positions x the C / groups
    channels of a group; ``groups=1`` is whole-sample layer norm, ``groups=-1`` instance norm (groups = C)."""
    _prefix = "group_normalization"

    def __init__(self, groups=32, axis=-1, epsilon=1e-3, center=True, scale=True, beta_initializer="zeros",
                 gamma_initializer="ones", beta_regularizer=None, gamma_regularizer=None, **kw):
        super().__init__(**kw)
        if isinstance(axis, (list, tuple)) or int(groups) == 0 or int(groups) < -1:
            raise ValueError(f"GroupNormalization: groups={groups!r}, axis={axis!r}")
        self.groups = int(groups)
        self._init_norm(axis, epsilon, center, scale, beta_initializer, gamma_initializer, beta_regularizer,
                        gamma_regularizer)

    def build(self, input_shape):
        self._check_axis(input_shape)
        c = input_shape[-1]
        if self.groups != -1 and c % self.groups:
            raise ValueError(f"{self.name}: groups={self.groups} does not divide the {c} channels")
        self._add_affine(c)
        self.built = True

    def n_groups(self, c):
        return c if self.groups == -1 else self.groups

    def ref_call(self, x, W, training, rng=None, state_updates=None):
        xc = x.movedim(-1, 1)
        return F.group_norm(xc, self.n_groups(x.shape[-1]), W.get("gamma"), W.get("beta"),
                            self.epsilon).movedim(1, -1)

    def get_config(self):
        return dict(groups=self.groups, **self._norm_config())


class LayerNormalization(_GroupNormBase):
    """Keras ``LayerNormalization`` over the last axis: every position of every sample is normalised over its C
    channels (``gamma``, ``beta`` [C])."""
    _prefix = "layer_normalization"

    def __init__(self, axis=-1, epsilon=1e-3, center=True, scale=True, beta_initializer="zeros",
                 gamma_initializer="ones", beta_regularizer=None, gamma_regularizer=None, **kw):
        super().__init__(**kw)
        if isinstance(axis, (list, tuple)):
            if len(axis) != 1:
                raise ValueError(f"LayerNormalization: axis={list(axis)!r}: only the last axis is supported (Keras "
                                 "would give gamma the shape of all listed axes); to normalise a whole sample use "
                                 "GroupNormalization(groups=1)")
            axis = axis[0]
        self._init_norm(axis, epsilon, center, scale, beta_initializer, gamma_initializer, beta_regularizer,
                        gamma_regularizer)

    def build(self, input_shape):
        self._check_axis(input_shape)
        self._add_affine(input_shape[-1])
        self.built = True

    def n_groups(self, c):
        return 1

    def ref_call(self, x, W, training, rng=None, state_updates=None):
        return F.layer_norm(x, x.shape[-1:], W.get("gamma"), W.get("beta"), self.epsilon)

    def get_config(self):
        return self._norm_config()


class MultiHeadAttention(Layer):
    """Keras ``MultiHeadAttention`` as self-attention: ``mha(x, x)`` or ``mha(x)`` on [N, T, D] or [N, H, W, D]
    (the T = H*W positions in row-major order are the tokens); the output has the input's shape.
        Q = x Wq + bq, K = x Wk + bk, V = x Wv + bv;  per head: O = softmax(Q K^T / sqrt(key_dim)) V;
        y = concat_heads(O) Wo + bo
    Weights in Keras's layout: ``query/kernel``, ``key/kernel`` [D, heads, key_dim], ``value/kernel``
    [D, heads, value_dim], their biases [heads, dim], ``attention_output/kernel`` [heads, value_dim, D] and
    ``attention_output/bias`` [D].  Cross-attention, masks, attention dropout and returned scores are refused.
    On the GPU: csrc/kernels/attention.hip between 1x1 GEMM stages (float32 policy)."""
    _prefix = "multi_head_attention"

    def __init__(self, num_heads, key_dim, value_dim=None, dropout=0.0, use_bias=True, output_shape=None,
                 attention_axes=None, kernel_initializer="glorot_uniform", bias_initializer="zeros",
                 kernel_regularizer=None, bias_regularizer=None, **kw):
        super().__init__(**kw)
        for arg, val, ok in (("dropout", dropout, dropout == 0), ("attention_axes", attention_axes,
                                                                  attention_axes is None),
                             ("output_shape", output_shape, output_shape is None)):
            if not ok:
                raise NotImplementedError(f"MultiHeadAttention: {arg}={val!r} is not supported")
        self.num_heads, self.key_dim = int(num_heads), int(key_dim)
        self.value_dim = int(value_dim) if value_dim is not None else self.key_dim
        if min(self.num_heads, self.key_dim, self.value_dim) < 1:
            raise ValueError(f"MultiHeadAttention: num_heads={num_heads!r}, key_dim={key_dim!r}, "
                             f"value_dim={value_dim!r}")
        self.use_bias = use_bias
        self.kernel_initializer, self.bias_initializer = kernel_initializer, bias_initializer
        self.kernel_regularizer = regularizers.get(kernel_regularizer)
        self.bias_regularizer = regularizers.get(bias_regularizer)

    def __call__(self, query, value=None, key=None, attention_mask=None, return_attention_scores=False,
                 training=None, use_causal_mask=False):
        for arg, bad in (("value", value is not None and value is not query), ("key", key is not None and
                                                                                 key is not query),
                         ("attention_mask", attention_mask is not None),
                         ("use_causal_mask", bool(use_causal_mask)),
                         ("return_attention_scores", bool(return_attention_scores))):
            if bad:
                raise NotImplementedError(f"{self.name} (MultiHeadAttention): {arg}= is not supported: "
                                          "self-attention only (mha(x, x)), no masks, no returned scores")
        return super().__call__(query)

    def projections(self):
        """(variable prefix, per-head size) of the three input projections, in Keras's weight order."""
        return (("query", self.key_dim), ("key", self.key_dim), ("value", self.value_dim))

    def build(self, input_shape):
        if len(input_shape) not in (2, 3):
            raise ValueError(f"{self.name}: input [N, T, D] or [N, H, W, D] expected, got {(None,) + tuple(input_shape)}")
        D, h = input_shape[-1], self.num_heads
        specs = [(n, (D, h, d), (h, d)) for n, d in self.projections()]
        for n, ks, bs in specs + [("attention_output", (h, self.value_dim, D), (D,))]:
            self.add_weight(f"{n}/kernel", ks, self.kernel_initializer, regularizer=self.kernel_regularizer)
            if self.use_bias:
                self.add_weight(f"{n}/bias", bs, self.bias_initializer, regularizer=self.bias_regularizer)
        self.built = True

    def ref_call(self, x, W, training, rng=None, state_updates=None):
        N, D, h = x.shape[0], x.shape[-1], self.num_heads
        xt = x.reshape(N, -1, D)

        def dense(t, n):
            k = W[f"{n}/kernel"]
            y = t @ (k.reshape(D, -1) if n != "attention_output" else k.reshape(-1, D))
            return y + W[f"{n}/bias"].reshape(-1) if self.use_bias else y

        q, k, v = (dense(xt, n).reshape(N, -1, h, d).transpose(1, 2) for n, d in self.projections())
        p = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(self.key_dim), dim=-1)
        o = (p @ v).transpose(1, 2).reshape(N, -1, h * self.value_dim)
        return dense(o, "attention_output").reshape(x.shape)

    def get_config(self):
        return dict(name=self.name, num_heads=self.num_heads, key_dim=self.key_dim, value_dim=self.value_dim,
                    use_bias=self.use_bias, **_reg_config(self, "kernel_regularizer", "bias_regularizer"))


def _unit_forget_bias(units, rest):
    """Keras's ``unit_forget_bias``: ones on the forget block [u:2u] of the [4u] bias, ``rest`` elsewhere."""
    def init(shape, gen):
        b = initializers.get(rest)(shape, gen).clone()
        b[units:2 * units] = 1.0
        return b
    return init


class LSTM(Layer):
    """Keras ``LSTM`` on [N, T, D]: the last h [N, units], or every h [N, T, units] with ``return_sequences``.
    From a zero state, with a_t = x_t W + b + h_{t-1} U in Keras's gate order i, f, c, o along the 4*units axis:
        i, f, o = sigmoid(a_i), sigmoid(a_f), sigmoid(a_o);  g = tanh(a_c)
        c_t = f * c_{t-1} + i * g;  h_t = o * tanh(c_t)
    Weights under Keras's nested names: ``lstm_cell/kernel`` [D, 4u], ``lstm_cell/recurrent_kernel`` [u, 4u],
    ``lstm_cell/bias`` [4u].  Other activations, dropout, masks, initial and returned state, ``go_backwards``,
    ``stateful`` and ``unroll`` are refused.  On the GPU: a 1x1 GEMM stage for x W + b over all N*T tokens, then
    the resident sweep of csrc/kernels/lstm.hip (float32 policy)."""
    _prefix = "lstm"

    def __init__(self, units, activation="tanh", recurrent_activation="sigmoid", use_bias=True,
                 kernel_initializer="glorot_uniform", recurrent_initializer="orthogonal", bias_initializer="zeros",
                 unit_forget_bias=True, kernel_regularizer=None, recurrent_regularizer=None, bias_regularizer=None,
                 dropout=0.0, recurrent_dropout=0.0, return_sequences=False, return_state=False, go_backwards=False,
                 stateful=False, unroll=False, **kw):
        super().__init__(**kw)
        for arg, val, ok in (("activation", activation, activation == "tanh"),
                             ("recurrent_activation", recurrent_activation, recurrent_activation == "sigmoid"),
                             ("dropout", dropout, dropout == 0), ("recurrent_dropout", recurrent_dropout,
                                                                  recurrent_dropout == 0),
                             ("return_state", return_state, not return_state),
                             ("go_backwards", go_backwards, not go_backwards), ("stateful", stateful, not stateful),
                             ("unroll", unroll, not unroll)):
            if not ok:
                raise NotImplementedError(f"LSTM: {arg}={val!r} is not supported")
        self.units = int(units)
        if self.units < 1:
            raise ValueError(f"LSTM: units={units!r}")
        self.use_bias, self.unit_forget_bias = use_bias, unit_forget_bias
        self.return_sequences = bool(return_sequences)
        self.kernel_initializer, self.recurrent_initializer = kernel_initializer, recurrent_initializer
        self.bias_initializer = bias_initializer
        self.kernel_regularizer = regularizers.get(kernel_regularizer)
        self.recurrent_regularizer = regularizers.get(recurrent_regularizer)
        self.bias_regularizer = regularizers.get(bias_regularizer)

    def __call__(self, inputs, mask=None, training=None, initial_state=None):
        for arg, val in (("mask", mask), ("initial_state", initial_state)):
            if val is not None:
                raise NotImplementedError(f"{self.name} (LSTM): {arg}= is not supported: whole sequences from a "
                                          "zero state only")
        return super().__call__(inputs)

    def build(self, input_shape):
        if len(input_shape) != 2:
            raise ValueError(f"{self.name}: input [N, T, D] expected, got {(None,) + tuple(input_shape)}")
        u = self.units
        self.add_weight("lstm_cell/kernel", (input_shape[-1], 4 * u), self.kernel_initializer,
                        regularizer=self.kernel_regularizer)
        self.add_weight("lstm_cell/recurrent_kernel", (u, 4 * u), self.recurrent_initializer,
                        regularizer=self.recurrent_regularizer)
        if self.use_bias:
            init = _unit_forget_bias(u, self.bias_initializer) if self.unit_forget_bias else self.bias_initializer
            self.add_weight("lstm_cell/bias", (4 * u,), init, regularizer=self.bias_regularizer)
        self.built = True

    def compute_output_shape(self, s):
        return (s[0], self.units) if self.return_sequences else (self.units,)

    def ref_call(self, x, W, training, rng=None, state_updates=None):
        z = x @ W["lstm_cell/kernel"]
        if self.use_bias:
            z = z + W["lstm_cell/bias"]
        h = c = x.new_zeros(x.shape[0], self.units)
        hs = []
        for t in range(x.shape[1]):
            i, f, g, o = (z[:, t] + h @ W["lstm_cell/recurrent_kernel"]).split(self.units, dim=-1)
            c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
            h = torch.sigmoid(o) * torch.tanh(c)
            hs.append(h)
        return torch.stack(hs, 1) if self.return_sequences else h

    def get_config(self):
        return dict(name=self.name, units=self.units, use_bias=self.use_bias,
                    unit_forget_bias=self.unit_forget_bias, return_sequences=self.return_sequences,
                    **_reg_config(self, "kernel_regularizer", "recurrent_regularizer", "bias_regularizer"))


class GRU(Layer):
    """Keras ``GRU`` in its default ``reset_after=True`` form on [N, T, D]: the last h [N, units], or every h
    [N, T, units] with ``return_sequences``.  From a zero state, with X_t = x_t W + b[0] and R_t = h_{t-1} U + b[1]
    in Keras's gate order z, r, h along the 3*units axis:
        z = sigmoid(X_z + R_z);  r = sigmoid(X_r + R_r);  hh = tanh(X_h + r * R_h)
        h_t = z * h_{t-1} + (1 - z) * hh
    Weights under Keras's nested names: ``gru_cell/kernel`` [D, 3u], ``gru_cell/recurrent_kernel`` [u, 3u],
    ``gru_cell/bias`` [2, 3u] (row 0 the input bias, row 1 the recurrent bias).  ``reset_after=False``, other
    activations, dropout, masks, initial and returned state, ``go_backwards``, ``stateful`` and ``unroll`` are
    refused.  On the GPU: a 1x1 GEMM stage for x W + b[0] over all N*T tokens, then the resident sweep of
    csrc/kernels/gru.hip (float32 policy)."""
    _prefix = "gru"

    def __init__(self, units, activation="tanh", recurrent_activation="sigmoid", use_bias=True,
                 kernel_initializer="glorot_uniform", recurrent_initializer="orthogonal", bias_initializer="zeros",
                 kernel_regularizer=None, recurrent_regularizer=None, bias_regularizer=None, dropout=0.0,
                 recurrent_dropout=0.0, return_sequences=False, return_state=False, go_backwards=False,
                 stateful=False, unroll=False, reset_after=True, **kw):
        super().__init__(**kw)
        for arg, val, ok in (("reset_after", reset_after, bool(reset_after)),
                             ("activation", activation, activation == "tanh"),
                             ("recurrent_activation", recurrent_activation, recurrent_activation == "sigmoid"),
                             ("dropout", dropout, dropout == 0), ("recurrent_dropout", recurrent_dropout,
                                                                  recurrent_dropout == 0),
                             ("return_state", return_state, not return_state),
                             ("go_backwards", go_backwards, not go_backwards), ("stateful", stateful, not stateful),
                             ("unroll", unroll, not unroll)):
            if not ok:
                raise NotImplementedError(f"GRU: {arg}={val!r} is not supported")
        self.units = int(units)
        if self.units < 1:
            raise ValueError(f"GRU: units={units!r}")
        self.use_bias = use_bias
        self.return_sequences = bool(return_sequences)
        self.kernel_initializer, self.recurrent_initializer = kernel_initializer, recurrent_initializer
        self.bias_initializer = bias_initializer
        self.kernel_regularizer = regularizers.get(kernel_regularizer)
        self.recurrent_regularizer = regularizers.get(recurrent_regularizer)
        self.bias_regularizer = regularizers.get(bias_regularizer)

    def __call__(self, inputs, mask=None, training=None, initial_state=None):
        for arg, val in (("mask", mask), ("initial_state", initial_state)):
            if val is not None:
                raise NotImplementedError(f"{self.name} (GRU): {arg}= is not supported: whole sequences from a "
                                          "zero state only")
        return super().__call__(inputs)

    def build(self, input_shape):
        if len(input_shape) != 2:
            raise ValueError(f"{self.name}: input [N, T, D] expected, got {(None,) + tuple(input_shape)}")
        u = self.units
        self.add_weight("gru_cell/kernel", (input_shape[-1], 3 * u), self.kernel_initializer,
                        regularizer=self.kernel_regularizer)
        self.add_weight("gru_cell/recurrent_kernel", (u, 3 * u), self.recurrent_initializer,
                        regularizer=self.recurrent_regularizer)
        if self.use_bias:
            self.add_weight("gru_cell/bias", (2, 3 * u), self.bias_initializer, regularizer=self.bias_regularizer)
        self.built = True

    def compute_output_shape(self, s):
        return (s[0], self.units) if self.return_sequences else (self.units,)

    @staticmethod
    def recurrence(X, U, rb, return_sequences):
        """The step loop over the projected input X [N, T, 3u] with the recurrent kernel U [u, 3u] and the
        recurrent bias rb [3u] (or None): every h [N, T, u], or the last [N, u]."""
        u = U.shape[0]
        h = X.new_zeros(X.shape[0], u)
        hs = []
        for t in range(X.shape[1]):
            R = h @ U if rb is None else h @ U + rb
            (xz, xr, xh), (rz, rr, rh) = X[:, t].split(u, dim=-1), R.split(u, dim=-1)
            z, r = torch.sigmoid(xz + rz), torch.sigmoid(xr + rr)
            h = z * h + (1 - z) * torch.tanh(xh + r * rh)
            hs.append(h)
        return torch.stack(hs, 1) if return_sequences else h

    def ref_call(self, x, W, training, rng=None, state_updates=None):
        X, b = x @ W["gru_cell/kernel"], W["gru_cell/bias"] if self.use_bias else None
        if b is not None:
            X = X + b[0]
        return self.recurrence(X, W["gru_cell/recurrent_kernel"], None if b is None else b[1], self.return_sequences)

    def get_config(self):
        return dict(name=self.name, units=self.units, use_bias=self.use_bias, reset_after=True,
                    return_sequences=self.return_sequences,
                    **_reg_config(self, "kernel_regularizer", "recurrent_regularizer", "bias_regularizer"))


class Bidirectional(Layer):
    """Keras ``Bidirectional`` around an ``LSTM`` or ``GRU`` of this module, ``merge_mode="concat"``: the wrapped
    recurrence over the sequence as it is and a second one, with weights of its own, over the reversed sequence;
    [N, T, 2u] with the wrapped layer's ``return_sequences`` (both halves in the original time order), else the two
    final states [N, 2u].  The weights are the wrapped layer's specs twice, under Keras's nested names
    ``forward_<inner>/<cell>/kernel`` ... and ``backward_<inner>/...``; initializers, regularizers, ``use_bias`` and
    ``unit_forget_bias`` are the wrapped layer's.  Other merge modes, ``backward_layer=``, ``weights=``, other wrapped
    layers, masks and initial state are refused.  On the GPU: two 1x1 GEMM stages and ONE launch per sweep for both
    directions (the BI kernels of csrc/kernels/lstm.hip / gru.hip), each writing its half of the output in place
    (float32 policy)."""
    _prefix = "bidirectional"

    def __init__(self, layer, merge_mode="concat", weights=None, backward_layer=None, **kw):
        super().__init__(**kw)
        if isinstance(layer, dict):   # a nested config
            layer = from_config(layer["class_name"], layer["config"])
        for arg, val, ok in (("layer", layer, type(layer) in (LSTM, GRU) and not layer.built),
                             ("merge_mode", merge_mode, merge_mode == "concat"),
                             ("backward_layer", backward_layer, backward_layer is None),
                             ("weights", weights, weights is None)):
            if not ok:
                raise NotImplementedError(f"{self.name} (Bidirectional): {arg}={val!r} is not supported: an unbuilt "
                                          "LSTM or GRU of this package, merge_mode='concat', weights of its own")
        self.layer, self.merge_mode = layer, merge_mode
        self.units, self.use_bias, self.return_sequences = layer.units, layer.use_bias, layer.return_sequences
        self.cell = f"{layer._prefix}_cell"
        self.prefixes = (f"forward_{layer.name}", f"backward_{layer.name}")   # direction 0, direction 1

    def __call__(self, inputs, mask=None, training=None, initial_state=None):
        for arg, val in (("mask", mask), ("initial_state", initial_state)):
            if val is not None:
                raise NotImplementedError(f"{self.name} (Bidirectional): {arg}= is not supported: whole sequences "
                                          "from a zero state only")
        return super().__call__(inputs)

    def build(self, input_shape):
        self.layer.build(input_shape)
        for pre in self.prefixes:
            for s in self.layer.weight_specs:
                self.weight_specs.append(WeightSpec(f"{pre}/{s.name}", s.shape, s.initializer,
                                                    s.trainable and self.trainable, s.aggregation, self, s.l1, s.l2))
        self.built = True

    def compute_output_shape(self, s):
        return (s[0], 2 * self.units) if self.return_sequences else (2 * self.units,)

    def ref_call(self, x, W, training, rng=None, state_updates=None):
        fw, bw = ({k[len(pre) + 1:]: v for k, v in W.items() if k.startswith(pre + "/")} for pre in self.prefixes)
        a = self.layer.ref_call(x, fw, training)
        b = self.layer.ref_call(torch.flip(x, [1]), bw, training)
        return torch.cat([a, torch.flip(b, [1]) if self.return_sequences else b], dim=-1)

    def get_config(self):   # ``from_config`` hands the nested config back to the constructor as ``layer``
        return dict(name=self.name, merge_mode=self.merge_mode,
                    layer={"class_name": type(self.layer).__name__, "config": self.layer.get_config()})


class Embedding(Layer):
    """Keras ``Embedding``: integer ids [N, T] -> [N, T, output_dim], rows of the one variable ``embeddings``
    [input_dim, output_dim].  Ids arrive as the model input (float32 on the device, truncated toward zero as Keras
    casts them to int32); an id outside [0, input_dim) gives a zero row and no gradient, as TensorFlow's GPU
    gather.  ``mask_zero``, ``embeddings_constraint``, ``sparse`` and ``lora_rank`` are refused.  On the GPU:
    the gather and the ordered scatter-sum of csrc/kernels/embedding.hip (float32 policy), first layer only."""
    _prefix = "embedding"

    def __init__(self, input_dim, output_dim, embeddings_initializer="uniform", embeddings_regularizer=None,
                 embeddings_constraint=None, mask_zero=False, input_length=None, sparse=False, lora_rank=None,
                 **kw):
        if input_length is not None and kw.get("input_shape") is None:
            kw["input_shape"] = (int(input_length),)
        super().__init__(**kw)
        for arg, val, ok in (("mask_zero", mask_zero, not mask_zero),
                             ("embeddings_constraint", embeddings_constraint, embeddings_constraint is None),
                             ("sparse", sparse, not sparse), ("lora_rank", lora_rank, lora_rank is None)):
            if not ok:
                raise NotImplementedError(f"Embedding: {arg}={val!r} is not supported")
        self.input_dim, self.output_dim = int(input_dim), int(output_dim)
        if min(self.input_dim, self.output_dim) < 1:
            raise ValueError(f"Embedding: input_dim={input_dim!r}, output_dim={output_dim!r}")
        self.input_length = None if input_length is None else int(input_length)
        self.embeddings_initializer = embeddings_initializer
        self.embeddings_regularizer = regularizers.get(embeddings_regularizer)

    def build(self, input_shape):
        if len(input_shape) != 1:
            raise ValueError(f"{self.name}: input [N, T] expected, got {(None,) + tuple(input_shape)}")
        self.add_weight("embeddings", (self.input_dim, self.output_dim), self.embeddings_initializer,
                        regularizer=self.embeddings_regularizer)
        self.built = True

    def compute_output_shape(self, s):
        return (s[0], self.output_dim)

    @staticmethod
    def lookup(ids, table):
        """table[ids] with the ids truncated toward zero and zero rows for those outside the table."""
        ids = ids.long()
        ok = (ids >= 0) & (ids < table.shape[0])
        return F.embedding(ids.clamp(0, table.shape[0] - 1), table) * ok.unsqueeze(-1).to(table.dtype)

    def ref_call(self, x, W, training, rng=None, state_updates=None):
        return self.lookup(x, W["embeddings"])

    def get_config(self):
        cfg = dict(name=self.name, input_dim=self.input_dim, output_dim=self.output_dim,
                   **_reg_config(self, "embeddings_regularizer"))
        if self.input_length is not None:
            cfg["input_length"] = self.input_length
        return cfg


class Add(Layer):
    """Element-wise sum of same-shaped inputs (ResNet shortcut join)."""
    _prefix = "add"
    multi_input = True

    def compute_output_shape(self, shapes):
        for s_ in shapes[1:]:
            if tuple(s_) != tuple(shapes[0]):
                raise ValueError(f"{self.name}: shape mismatch {shapes}")
        return tuple(shapes[0])

    def ref_call(self, xs, W, training, rng=None, state_updates=None):
        out = xs[0]
        for x in xs[1:]:
            out = out + x
        return out


class InputStageLayer(Layer):
    """A random image transform of the model's input stage: the unbroken chain of such layers directly behind
    the model input.  No weights, shape preserved, the identity whenever the learning phase is not training.
    No plan runs these layers: the launch that fills the training program's input ring applies them
    (``csrc/kernels/augment.hip``; host twin ``ops/augment.py``), as a pure function of (seed, global step,
    index in the stage, local row), and the plans see the model without them (``Model._nodes``)."""
    _seed_base = 104729   # make_generator(_seed_base + j) draws the seed of a layer built without one

    def compute_output_shape(self, s):
        if len(s) != 3:
            raise ValueError(f"{self.name}: expects channels_last images (H, W, C), got shape {tuple(s)}")
        return tuple(s)

    def ref_call(self, x, W, training, rng=None, state_updates=None):
        return x   # the direct call runs inference ops

    def resolved_seed(self, j):
        """The Philox key of this layer at index ``j`` of the input stage."""
        if self.seed is not None:
            return int(self.seed)
        g = K.make_generator(self._seed_base + j)
        return int(torch.randint(0, 2 ** 62, (1,), generator=g).item())


class RandomFlip(InputStageLayer):
    _prefix = "random_flip"
    MODES = ("horizontal", "vertical", "horizontal_and_vertical")

    def __init__(self, mode="horizontal_and_vertical", seed=None, **kw):
        super().__init__(**kw)
        if mode not in self.MODES:
            raise ValueError(f"RandomFlip: mode must be one of {self.MODES}, got {mode!r}")
        self.mode = mode
        self.seed = None if seed is None else int(seed)

    def aug_layer(self, j):
        from ..ops import augment as AU
        return AU.flip_layer(self.mode, j, self.resolved_seed(j))

    def get_config(self):
        return dict(name=self.name, mode=self.mode, seed=self.seed)


def _translation_factor(v, what, who="RandomTranslation"):
    """A factor f >= 0 (the range [-f, f]) or a pair (lo, hi) with -1 <= lo <= hi <= 1 -> (lo, hi)."""
    if isinstance(v, (tuple, list)):
        if len(v) != 2:
            raise ValueError(f"{who}: {what} must be a float or a (lo, hi) pair, got {v!r}")
        lo, hi = float(v[0]), float(v[1])
    elif isinstance(v, (int, float)) and not isinstance(v, bool):
        if v < 0:
            raise ValueError(f"{who}: {what} must not be negative, got {v!r}")
        lo, hi = -float(v), float(v)
    else:
        raise ValueError(f"{who}: {what} must be a float or a (lo, hi) pair, got {v!r}")
    if not (-1.0 <= lo <= hi <= 1.0):
        raise ValueError(f"{who}: {what} needs -1 <= lo <= hi <= 1, got {v!r}")
    return lo, hi


class RandomTranslation(InputStageLayer):
    _prefix = "random_translation"
    FILL_MODES = ("constant", "nearest", "reflect", "wrap")
    INTERPOLATIONS = ("nearest", "bilinear")

    def __init__(self, height_factor, width_factor, fill_mode="reflect", interpolation="bilinear", seed=None,
                 fill_value=0.0, **kw):
        super().__init__(**kw)
        self.height_factor = tuple(height_factor) if isinstance(height_factor, (tuple, list)) else height_factor
        self.width_factor = tuple(width_factor) if isinstance(width_factor, (tuple, list)) else width_factor
        self.height_range = _translation_factor(height_factor, "height_factor")
        self.width_range = _translation_factor(width_factor, "width_factor")
        if fill_mode not in self.FILL_MODES:
            raise ValueError(f"RandomTranslation: fill_mode must be one of {self.FILL_MODES}, got {fill_mode!r}")
        if interpolation not in self.INTERPOLATIONS:
            raise ValueError(f"RandomTranslation: interpolation must be one of {self.INTERPOLATIONS}, "
                             f"got {interpolation!r}")
        self.fill_mode = fill_mode
        self.interpolation = interpolation
        self.seed = None if seed is None else int(seed)
        self.fill_value = float(fill_value)

    def aug_layer(self, j):
        from ..ops import augment as AU
        return AU.translate_layer(self.height_range, self.width_range, self.fill_mode, self.interpolation,
                                  self.fill_value, j, self.resolved_seed(j))

    def get_config(self):
        return dict(name=self.name, height_factor=self.height_factor, width_factor=self.width_factor,
                    fill_mode=self.fill_mode, interpolation=self.interpolation, seed=self.seed,
                    fill_value=self.fill_value)


class _RandomAffine(InputStageLayer):
    """What RandomRotation and RandomZoom share: the translation's fill modes and interpolations."""
    FILL_MODES = RandomTranslation.FILL_MODES
    INTERPOLATIONS = RandomTranslation.INTERPOLATIONS

    def _sampling(self, fill_mode, interpolation, seed, fill_value):
        who = type(self).__name__
        if fill_mode not in self.FILL_MODES:
            raise ValueError(f"{who}: fill_mode must be one of {self.FILL_MODES}, got {fill_mode!r}")
        if interpolation not in self.INTERPOLATIONS:
            raise ValueError(f"{who}: interpolation must be one of {self.INTERPOLATIONS}, got {interpolation!r}")
        self.fill_mode = fill_mode
        self.interpolation = interpolation
        self.seed = None if seed is None else int(seed)
        self.fill_value = float(fill_value)


class RandomRotation(_RandomAffine):
    """Rotation about the image centre by a fraction of a full turn drawn from ``factor`` (a float f >= 0: the
    range [-f, f]; or a pair (lo, hi)); a positive value turns the picture counter-clockwise as displayed."""
    _prefix = "random_rotation"

    def __init__(self, factor, fill_mode="reflect", interpolation="bilinear", seed=None, fill_value=0.0, **kw):
        super().__init__(**kw)
        self.factor = tuple(factor) if isinstance(factor, (tuple, list)) else factor
        self.factor_range = _translation_factor(factor, "factor", "RandomRotation")
        self._sampling(fill_mode, interpolation, seed, fill_value)

    def aug_layer(self, j):
        from ..ops import augment as AU
        return AU.rotate_layer(self.factor_range, self.fill_mode, self.interpolation, self.fill_value, j,
                               self.resolved_seed(j))

    def get_config(self):
        return dict(name=self.name, factor=self.factor, fill_mode=self.fill_mode, interpolation=self.interpolation,
                    seed=self.seed, fill_value=self.fill_value)


class RandomZoom(_RandomAffine):
    """Zoom about the image centre: an axis is scaled by 1 + f with f drawn from its factor's range, positive
    zooming out and negative in.  ``width_factor=None``: the width takes the height's drawn value (the aspect
    ratio is kept)."""
    _prefix = "random_zoom"

    def __init__(self, height_factor, width_factor=None, fill_mode="reflect", interpolation="bilinear", seed=None,
                 fill_value=0.0, **kw):
        super().__init__(**kw)
        self.height_factor = tuple(height_factor) if isinstance(height_factor, (tuple, list)) else height_factor
        self.width_factor = tuple(width_factor) if isinstance(width_factor, (tuple, list)) else width_factor
        self.height_range = _translation_factor(height_factor, "height_factor", "RandomZoom")
        self.width_range = None if width_factor is None else _translation_factor(width_factor, "width_factor",
                                                                                 "RandomZoom")
        self._sampling(fill_mode, interpolation, seed, fill_value)

    def aug_layer(self, j):
        from ..ops import augment as AU
        return AU.zoom_layer(self.height_range, self.width_range, self.fill_mode, self.interpolation, self.fill_value,
                             j, self.resolved_seed(j))

    def get_config(self):
        return dict(name=self.name, height_factor=self.height_factor, width_factor=self.width_factor,
                    fill_mode=self.fill_mode, interpolation=self.interpolation, seed=self.seed,
                    fill_value=self.fill_value)


LAYER_CLASSES = {c.__name__: c for c in [InputLayer, Conv2D, DepthwiseConv2D, SeparableConv2D, Dense, MaxPooling2D, AveragePooling2D,
                                         GlobalAveragePooling2D, GlobalAveragePooling1D, ZeroPadding2D, Flatten, Reshape, Activation, ReLU,
                                         Dropout, BatchNormalization, GroupNormalization,
                                         LayerNormalization, MultiHeadAttention, LSTM, GRU, Bidirectional, Embedding, Add,
                                         RandomFlip,
                                         RandomTranslation, RandomRotation, RandomZoom]}


def from_config(cls_name, cfg):
    cfg = dict(cfg)
    cls = LAYER_CLASSES[cls_name]
    return cls(**cfg)

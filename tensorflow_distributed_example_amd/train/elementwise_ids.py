"""Layer ids and dropout seeds of a model's element-wise stages, shared by every plan that draws
Philox dropout masks (``train/layerwise.py``, ``train/smallnet.py``).

A mask is ``philox_keep(rate, seed, step, lid, element)`` (``csrc/include/tde_philox.h``,
``ops/philox.py``).  ``lid`` is the running count of element-wise stages of the model's node list: every
BatchNormalization / Activation / Dropout / Add that is not absorbed into the stage in front of it opens a
stage, and a stage absorbs the ``[Add] [ReLU] [Dropout]`` chain that follows it (a Dropout absorbed into an
``Activation("relu")`` stage takes that stage's id).  The seed is the layer's own, else a draw from
``make_generator(7919 + lid)``.  One derivation for every plan, so a model trains through the same masks
whichever plan runs it.
"""
from __future__ import annotations

import torch

from .. import backend as Kb
from ..models import layers as L


def _is_relu(layer):
    return isinstance(layer, L.Activation) and layer.activation == "relu"


def elementwise_chains(nodes):
    """``{node index: dict(lid, add, relu, drop)}`` for every node that opens an element-wise stage;
    ``add`` / ``relu`` / ``drop`` are the indices of the nodes the stage absorbs (or None).  ``nodes`` is
    ``model._nodes()``; the last node is the head and opens no stage."""
    consumers = {0: []}
    for i, (_, ins, out) in enumerate(nodes):
        consumers.setdefault(out, [])
        for j in ins:
            consumers[j].append(i)

    def single(t):
        return consumers[t][0] if len(consumers[t]) == 1 else None

    chains = {}
    fused = set()
    lid = 0
    for i, (layer, ins, out) in enumerate(nodes):
        if i in fused or i == len(nodes) - 1:
            continue
        if not isinstance(layer, (L.BatchNormalization, L.Activation, L.Dropout, L.Add)):
            continue
        ch = dict(lid=lid, add=None, relu=None, drop=None)
        lid += 1
        cur = out
        if isinstance(layer, L.BatchNormalization):
            k = single(cur)
            if (k is not None and isinstance(nodes[k][0], L.Add) and len(nodes[k][1]) == 2 and k not in fused
                    and len([j for j in nodes[k][1] if j != out]) == 1):
                ch["add"] = k
                fused.add(k)
                cur = nodes[k][2]
        if not isinstance(layer, (L.Dropout, L.Activation)):
            k = single(cur)
            if k is not None and _is_relu(nodes[k][0]):
                ch["relu"] = k
                fused.add(k)
                cur = nodes[k][2]
        if not isinstance(layer, L.Dropout):
            k = single(cur)
            if k is not None and isinstance(nodes[k][0], L.Dropout):
                ch["drop"] = k
                fused.add(k)
        chains[i] = ch
    return chains


def dropout_seed(layer, lid):
    """The Philox key of Dropout ``layer`` in the stage with id ``lid``."""
    g = Kb.make_generator(7919 + lid)
    return int(torch.randint(0, 2 ** 62, (1,), generator=g).item()) if layer.seed is None else int(layer.seed)


def dropout_ids(model):
    """``{Dropout layer name: (lid, seed)}`` of every Dropout of ``model`` in front of its head."""
    nodes = model._nodes()
    out = {}
    for i, ch in elementwise_chains(nodes).items():
        k = i if isinstance(nodes[i][0], L.Dropout) else ch["drop"]
        if k is not None:
            layer = nodes[k][0]
            out[layer.name] = (ch["lid"], dropout_seed(layer, ch["lid"]))
    return out

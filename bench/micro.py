#!/usr/bin/env python
"""Kernel microbenchmarks for the fused MNIST-CNN plan on one MI355X.

* launch floor: empty-kernel cost, eager and inside a hipGraph;
* per-kernel standalone time: each kernel of the step replayed 200x in a graph;
* phase stamps: s_memrealtime stamps at phase boundaries of each workgroup
  (diagnostic only) -> where inside each kernel the time goes.  The float32 kernels given a stamp buffer
  are the general forms (csrc/kernels/convnet_f32.hip): the stamps locate the phases, the graph times above
  them (no stamp buffer) are the production forms'.
* hand-off between the two launches of the fused step (``--handoff``: that section alone): the fused kernels
  following themselves and alternating, the alternating pair with one operand at a time read from a second copy
  that the other launch does not write (W1 by the forward; Pt with amax, and hpre, by the backward), the pair under
  the identity placement maps, and the XCD of every workgroup of both kernels, eager and in a replayed graph.
Prints one JSON object; used to build profiles/*.md.
"""
from __future__ import annotations

import json
import sys

import os
sys_path_root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
import sys as _sys
_sys.path.insert(0, sys_path_root)
import numpy as np
import torch


def graph_time(fn, reps=200, inner=1):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = 1e9
    for _ in range(5):
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e3 / reps)
    return best


def eager_time(fn, reps=500):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def stamps_summary(st, slots):
    """Per slot (a column of ``st``) min / median / max over the workgroups that wrote all of ``slots``, from the
    earliest workgroup's slot 0.  Slots no workgroup wrote (a library without them) are left out."""
    st = np.asarray(st, dtype=np.float64)
    slots = [i for i in (range(slots) if isinstance(slots, int) else slots) if (st[:, i] > 0).any()]
    used = st[:, slots]
    used = used[(used > 0).all(axis=1)]
    if len(used) == 0:
        return {}
    t0 = used[:, 0].min()
    rel = (used - t0) * 0.01  # 100 MHz ticks -> us
    return {f"slot{s}": {"min": round(float(rel[:, k].min()), 2), "med": round(float(np.median(rel[:, k])), 2),
                         "max": round(float(rel[:, k].max()), 2)} for k, s in enumerate(slots)}


# the float32 backward's slots in time order: 8..12 (operands landed, staging barrier passed, logit partials
# published, dlogits published, G / G^T stored) are its second bank of 8, which lies behind the first bank of
# all workgroups (csrc/include/tde_convnet.h: stamp_fine)
BWD_SLOTS = [0, 1, 8, 9, 10, 11, 12, 2, 3, 4, 5]


def xcd_table(plan, k_fwd, k_bwd, ngroups, ntiles):
    """HW_REG_XCC_ID of every workgroup of the two (general-form) kernels, from stamp slot 6 (id + 1; 0: not
    written): one eager launch each, then three replays of one graph holding both."""
    nf, nb = ngroups * ntiles, plan.P + 1
    sf = torch.zeros(4096 * 8, dtype=torch.int64, device="cuda")
    sb = torch.zeros(4096 * 8, dtype=torch.int64, device="cuda")

    def both():
        k_fwd(stamps=sf)
        k_bwd(stamps=sb)

    def read():
        f = (sf.view(-1, 8)[:nf, 6] - 1).cpu().tolist()
        b = (sb.view(-1, 8)[:nb, 6] - 1).cpu().tolist()
        sf.zero_()
        sb.zero_()
        return {"fwd": f, "bwd": b}

    def summary(t):
        r = {}
        for n, v in t.items():
            r[n + "_b_and_b8_share"] = all(v[i] == v[i + 8] for i in range(len(v) - 8))
            r[n + "_class_xcd"] = v[:8]
        r["class_xcd_equal_in_both_launches"] = t["fwd"][:8] == t["bwd"][:8]
        return r

    both()
    torch.cuda.synchronize()
    sf.zero_()
    sb.zero_()
    both()
    torch.cuda.synchronize()
    eager = read()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        both()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        both()
    replays = []
    for _ in range(3):
        sf.zero_()
        sb.zero_()
        g.replay()
        torch.cuda.synchronize()
        replays.append(read())
    return {"eager": eager, "eager_summary": summary(eager), "graph_replays": replays,
            "graph_summary": [summary(t) for t in replays]}


def handoff(plan, k_fwd, k_bwd, x, y, rounds=3):
    """The fused step's two launches in graphs of 200 nodes, no stamp buffer (the production forms)."""
    from tensorflow_distributed_example_amd import _native as N
    ident = getattr(N.hip(), "tde_convnet_f32_identity_slots", None)
    plan.set_step_mode("local")
    for _ in range(4):   # real contents for the second copies
        plan.train_step(x, y)
    torch.cuda.synchronize()
    W1c, Ptc, amc = plan.W1fwd.clone(), plan.Pt.clone(), plan.amax.clone()
    hc = (torch.randn_like(plan.hpre2[0]) * 0.1).contiguous()

    def pair(**kw):
        def fn():
            k_fwd(W1=kw.get("W1"))
            k_bwd(Pt=kw.get("Pt"), amax=kw.get("amax"), hpre=kw.get("hpre"))
            plan.parity = 1 - plan.parity
        return fn

    variants = [("pair", {}), ("pair_warm_W1", dict(W1=W1c)), ("pair_warm_Pt_amax", dict(Pt=Ptc, amax=amc)),
                ("pair_warm_hpre", dict(hpre=hc)), ("pair_warm_all", dict(W1=W1c, Pt=Ptc, amax=amc, hpre=hc))]
    res = {n: [] for n, _ in variants}
    res.update(fwd_after_fwd=[], bwd_after_bwd=[])
    if ident is not None:
        res["pair_identity_slots"] = []
    for _ in range(rounds):
        res["fwd_after_fwd"].append(graph_time(k_fwd, reps=200))
        res["bwd_after_bwd"].append(graph_time(k_bwd, reps=200))
        for n, kw in variants:
            res[n].append(graph_time(pair(**kw), reps=100))
        if ident is not None:
            prev = ident(1)
            res["pair_identity_slots"].append(graph_time(pair(), reps=100))
            ident(prev)
    plan.finish()
    med = {n: float(np.median(v)) for n, v in res.items()}
    res["median"] = med
    res["pair_minus_self_loops"] = med["pair"] - med["fwd_after_fwd"] - med["bwd_after_bwd"]
    res["added_by"] = {"W1": med["pair"] - med["pair_warm_W1"], "Pt_amax": med["pair"] - med["pair_warm_Pt_amax"],
                       "hpre": med["pair"] - med["pair_warm_hpre"], "all": med["pair"] - med["pair_warm_all"]}
    res["pair_spread"] = max(res["pair"]) - min(res["pair"])
    return res


def main():
    only_handoff = "--handoff" in sys.argv[1:]
    import tensorflow_distributed_example_amd as tde
    from tensorflow_distributed_example_amd.ops import kernels as K
    torch.cuda.set_device(0)
    out = {}
    if not only_handoff:
        noop_floor(K, out)
    tde.backend.set_random_seed(0)
    m = tde.zoo.mnist_cnn()
    m.compile(loss=tde.losses.SparseCategoricalCrossentropy(from_logits=True), optimizer=tde.optimizers.SGD(0.001),
              metrics=["accuracy"])
    prog = m._program("train", 64)
    plan = prog.plans[0]
    x = torch.rand(64, 28, 28, 1, device="cuda")
    y = torch.randint(0, 10, (64,), device="cuda", dtype=torch.int32)

    def k_fwd(stamps=None, W1=None):
        q = plan.parity
        local = plan.step_mode == "local"
        K.convnet_fwd(x, plan._v("wc"), plan._v("bc"), plan.W1fwd if W1 is None else W1, plan.hpre2[q], plan.Pt,
                      plan.amax, stamps=stamps, opt=plan._fopt[q] if local else None,
                      off_wc=plan.store.segments[plan.names["wc"]].offset,
                      off_bc=plan.store.segments[plan.names["bc"]].offset, inc_iter=plan.iterations,
                      hrep=plan.hrep)

    def k_bwd(stamps=None, Pt=None, amax=None, hpre=None):
        q = plan.parity
        local = plan.step_mode == "local"
        dwc, dbc, _ = plan._conv_grads(q)
        K.convnet_bwd(x, plan.amax if amax is None else amax, plan.hpre2[q] if hpre is None else hpre,
                      plan.hpre2[1 - q], plan._v("b1"), plan._v("w2"), plan._v("b2"), y,
                      scale=plan.scale, pre_relu=True, metrics=plan.metrics, W1row=plan.W1row,
                      Pt=plan.Pt if Pt is None else Pt,
                      dW1=plan._g("w1"), dwc=dwc, dbc=dbc, dW2=plan._g("w2"), db2=plan._g("b2"), db1=plan._g("b1"),
                      B=64, stamps=stamps, opt=plan._bopt[q] if local else None)

    if not only_handoff:
        kernels_and_stamps(plan, K, x, y, k_fwd, k_bwd, out)
    out["handoff_us"] = handoff(plan, k_fwd, k_bwd, x, y)
    plan.set_step_mode("plain")
    out["xcd"] = xcd_table(plan, k_fwd, k_bwd, (plan.P + 3) // 4, 4)
    print(json.dumps(out, indent=1))


def noop_floor(K, out):
    out["noop_eager_us"] = eager_time(lambda: K.noop(1, 64))
    out["noop_graph_us"] = graph_time(lambda: K.noop(1, 64))
    out["noop_graph_256wg_us"] = graph_time(lambda: K.noop(256, 256))
    out["noop_graph_1024thr_43wg_us"] = graph_time(lambda: K.noop(43, 1024))


def kernels_and_stamps(plan, K, x, y, k_fwd, k_bwd, out):
    def k_opt():
        plan.opt.apply()

    def step():
        plan.train_step(x, y)
        plan.apply()

    def step_local():
        plan.train_step(x, y)

    plan.set_step_mode("plain")
    out["w1_source"] = "rows" if plan.w1_rows else "col"
    out["kernel_graph_us"] = {n: graph_time(f) for n, f in
                              [("convnet_fwd", k_fwd), ("convnet_bwd_head", k_bwd), ("optim", k_opt)]}
    out["step_graph_us"] = graph_time(step, reps=100)
    out["step_eager_us"] = eager_time(step, reps=200)
    # fused single-replica step: the optimizer inside the two launches, one flush per execution
    plan.set_step_mode("local")
    out["local_kernel_graph_us"] = {n: graph_time(f) for n, f in
                                    [("convnet_fwd", k_fwd), ("convnet_bwd_head", k_bwd), ("flush", plan.finish)]}
    out["local_step_graph_us"] = graph_time(step_local, reps=100)
    plan.finish()
    plan.set_step_mode("plain")
    st = torch.zeros(4096 * 8, dtype=torch.int64, device="cuda")
    nwg_bwd = plan.P + 1   # 16 slots per workgroup of the backward: 2 banks x 8, 4096 x 8 values hold both
    for name, f, ns in [("convnet_fwd", k_fwd, 5), ("convnet_bwd_head", k_bwd, BWD_SLOTS)]:
        st.zero_()
        f()
        torch.cuda.synchronize()
        st.zero_()
        f(stamps=st)
        torch.cuda.synchronize()
        rows = st.view(-1, 8).cpu().numpy().astype(np.float64)
        if name == "convnet_bwd_head":
            rows = np.concatenate([rows[:nwg_bwd], rows[nwg_bwd:2 * nwg_bwd]], axis=1)
        out[f"stamps_{name}"] = stamps_summary(rows, ns)
        head = rows[rows[:, 7] > 0]
        if len(head):   # the backward's head workgroup: start and end, on the trunk's clock
            t0 = rows[rows[:, 0] > 0, 0].min()
            out[f"stamps_{name}_head_wg"] = {"start": round((head[0, 0] - t0) * 0.01, 2),
                                            "end": round((head[0, 7] - t0) * 0.01, 2)}


if __name__ == "__main__":
    main()

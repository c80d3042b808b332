"""Child process of tests/test_smallnet_act_gpu.py: ``lenet5_classic`` (tanh, average pooling; both convs
on the compile-time geometries) and ``dgrad_tanh`` (a compile-time-geometry conv fed by a tanh conv) under
the TDE_SN_MFMA mask of this process's environment -- the library reads it once, at the first step, so a
mask other than the default needs a fresh process.  Prints one line ``SMALLNET_ACT <json>``: the figures of
``smallnet_act_oracle.measure``."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import smallnet_act_oracle as A
    import tensorflow_distributed_example_amd as tde
    figs = []
    for name in A.FAST:
        tde.backend.clear_session()
        figs.append(A.measure(tde, name, *A.O.FAST_BATCH))
    print("SMALLNET_ACT " + json.dumps(dict(mask=os.environ.get("TDE_SN_MFMA"), figs=figs)), flush=True)


if __name__ == "__main__":
    main()

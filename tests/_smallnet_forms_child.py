"""Child process of tests/test_smallnet_forms_gpu.py: the compile-time-geometry models under the
TDE_SN_MFMA mask of this process's environment (the library reads it once, at the first step, so a mask
other than the default needs a fresh process).  Prints one line ``SMALLNET_FORMS <json>``: the figures of
``smallnet_oracle.measure`` for lenet5, lenet5_nobias and geo3 on quantized data and for one lenet5 step
on unquantized randn data (whose conv-gradient hashes tell the parent that the mask took effect)."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import smallnet_oracle as O
    import tensorflow_distributed_example_amd as tde
    figs = []
    B, Bplan = O.FAST_BATCH
    for name, data in [(n, "grid") for n in O.FAST] + [("lenet5", "randn")]:
        tde.backend.clear_session()
        figs.append(O.measure(tde, name, B, Bplan, data))
    print("SMALLNET_FORMS " + json.dumps(dict(mask=os.environ.get("TDE_SN_MFMA"), figs=figs)), flush=True)


if __name__ == "__main__":
    main()

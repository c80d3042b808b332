"""Child process of tests/test_smallnet_forms_gpu.py and tests/test_smallnet_act_gpu.py (started by
tests/smallnet_child.py): the compile-time-geometry models of the suite named on the command line, ``forms``
or ``act``, under the TDE_SN_MFMA mask of this process's environment -- the library reads it once, at the
first step, so a mask other than the default needs a fresh process.  Prints one line
``SMALLNET_CHILD <json>``: the figures of ``smallnet_oracle.measure`` for the suite's FAST models at
FAST_BATCH and, in the forms suite, for one lenet5 step on unquantized randn data (whose conv-gradient
hashes tell the parent that the mask took effect)."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)


def main(suite):
    import smallnet_cases as C
    import smallnet_oracle as O
    import tensorflow_distributed_example_amd as tde
    figs = []
    for name, data in [(n, None) for n in C.FAST[suite]] + ([("lenet5", "randn")] if suite == "forms" else []):
        tde.backend.clear_session()
        figs.append(O.measure(tde, suite, name, *C.FAST_BATCH, data))
    print("SMALLNET_CHILD " + json.dumps(dict(suite=suite, mask=os.environ.get("TDE_SN_MFMA"), figs=figs)), flush=True)


if __name__ == "__main__":
    main(sys.argv[1])

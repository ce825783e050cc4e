"""infer.run_loop raises when its output cannot be written, in both loops.  The pipelined loop used to hang there: the writer
thread recorded its error and stopped taking items, and the main loop blocked for good on the writer's full queue four images
later (tests/test_pipeline_cpu.py holds the skeleton's side of this).  The failure is a host I/O error -- a directory that does
not exist -- and nothing on the device is provoked."""
import os
import threading

import pytest
import torch

from tests import abi_log_prep as A

pytestmark = pytest.mark.gpu


def test_unwritable_out_dir_raises_in_both_loops(tmp_path):
    from codon_amd import infer
    dd, cd, ld, _ = A.write_set(str(tmp_path / "set"), 8, 255, n=8)   # eight pairs: more than the writer's queue holds
    missing = str(tmp_path / "no" / "such" / "directory")
    dev = torch.device("cuda:0")
    raised = {}

    def run(pipelined):
        try:
            infer.run_loop(A.Stub(), dev, torch.float32, None, cd, dd, missing, pipelined=pipelined, emit=A.quiet, lr_depth=ld, scale=4)
        except BaseException as e:      # noqa: BLE001
            raised[pipelined] = e

    t = threading.Thread(target=run, args=(True,), name="test_pipelined_run_loop", daemon=True)
    t.start()
    t.join(60.0)                        # a condition, not a measurement: a hang fails here instead of stalling the session
    assert not t.is_alive(), "the pipelined run_loop hangs on a failing writer"
    assert not [x.name for x in threading.enumerate() if x.name.startswith("codon_infer_")]
    run(False)
    assert isinstance(raised.get(True), OSError), raised.get(True)
    assert type(raised.get(False)) is type(raised[True]), raised.get(False)
    assert not os.path.exists(missing)

"""codon_amd.pipeline.run_pipeline, the skeleton of infer's pipelined loop, with plain Python stages: the order of the stages, and
that a failure in any of them is raised in the caller with no thread of the pipeline left alive.  Every case runs in a helper
thread joined with a 30 s cap: a condition, not a measurement -- a hang fails the test instead of the session."""
import threading
import time

import pytest

from codon_amd.pipeline import run_pipeline

CAP = 30.0


class Boom(Exception):
    pass


def _alive():
    return [t.name for t in threading.enumerate() if t.name.startswith("pl_test_")]


def _run(n, readers=3, load=None, step=None, settle=None, write=None):
    """run_pipeline over range(n) in a helper thread -> (the event log [(stage, item), ...], the exception raised or None).
    The given stages run after the call is logged."""
    log, lock, raised = [], threading.Lock(), []

    def stage(tag, fn, out=lambda i: i):
        def f(i):
            with lock:
                log.append((tag, i))
            if fn is not None:
                fn(i)
            return out(i)
        return f

    def target():
        try:
            run_pipeline(list(range(n)), stage("load", load), stage("step", step, lambda i: (i, i)), stage("settle", settle),
                         stage("write", write), readers=readers, name="pl_test")
        except BaseException as e:      # noqa: BLE001
            raised.append(e)

    t = threading.Thread(target=target, name="pl_test_caller", daemon=True)
    t.start()
    t.join(CAP)
    assert not t.is_alive(), f"run_pipeline did not return within {CAP} s; alive: {_alive()}"
    assert _alive() == []
    return log, (raised[0] if raised else None)


def _of(log, tag):
    return [i for s, i in log if s == tag]


def _check_order(log, n):
    assert _of(log, "step") == list(range(n)) and _of(log, "write") == list(range(n))
    assert sorted(_of(log, "load")) == list(range(n))
    assert _of(log, "settle") == list(range(n))                      # each exactly once
    for i in range(n - 1):                                           # one item behind: step(i + 1) has started
        assert log.index(("settle", i)) > log.index(("step", i + 1))
    assert log.index(("settle", n - 1)) > log.index(("step", n - 1))


def test_order():
    log, e = _run(7, load=lambda i: time.sleep(0.002 * (7 - i)))
    assert e is None
    _check_order(log, 7)


@pytest.mark.parametrize("n,readers", [(7, 1), (2, 3), (1, 3)])
def test_one_reader_and_fewer_items_than_readers(n, readers):
    log, e = _run(n, readers=readers, load=lambda i: time.sleep(0.002 * (n - i)))
    assert e is None
    _check_order(log, n)


def test_threads_are_named_and_take_every_kth_item():
    seen = {}
    log, e = _run(7, load=lambda i: seen.setdefault(i, threading.current_thread().name),
                  write=lambda i: seen.setdefault("w", threading.current_thread().name))
    assert e is None
    assert seen == {**{i: f"pl_test_reader{i % 3}" for i in range(7)}, "w": "pl_test_writer"}


def test_reader_failure():
    def load(i):
        if i == 4:
            raise Boom("load 4")

    log, e = _run(16, load=load)
    assert isinstance(e, Boom) and str(e) == "load 4"
    assert _of(log, "step") == [0, 1, 2, 3]
    assert _of(log, "write") == [0, 1, 2, 3] and _of(log, "settle") == [0, 1, 2, 3]      # what was stepped is finished


def test_writer_failure():
    """Sixteen items are more than the queues hold (2 per reader, 4 to the writer): a caller that does not look at the
    writer's error, with a writer that stops taking items, blocks for good on its fifth put."""
    failed = threading.Event()

    def write(i):
        if i == 0:
            failed.set()
            raise Boom("write 0")

    def step(i):
        if i == 1:
            assert failed.wait(CAP)                                  # the writer's error is recorded after this, at once

    log, e = _run(16, step=step, write=write)
    assert isinstance(e, Boom) and str(e) == "write 0"
    assert _of(log, "step") in ([0, 1], [0, 1, 2])                   # item 1 was under way; at most one further step
    assert _of(log, "write") == [0]                                  # the failed writer empties its queue, it writes no more


def test_step_failure():
    def step(i):
        if i == 2:
            raise Boom("step 2")

    log, e = _run(16, step=step)
    assert isinstance(e, Boom) and str(e) == "step 2"
    assert _of(log, "step") == [0, 1, 2] and _of(log, "settle") == [0]
    assert _of(log, "write") == [0, 1]
    assert len(_of(log, "load")) < 16                                # the readers were stopped, not run to the end


def test_first_recorded_error_wins():
    def load(i):
        if i == 0:
            raise Boom("load 0")
        time.sleep(0.05)                                             # the other readers fail later, or are stopped
        raise Boom(f"load {i}")

    log, e = _run(6, load=load)
    assert str(e) == "load 0" and _of(log, "step") == []


def test_empty_list():
    log, e = _run(0)
    assert e is None and log == []

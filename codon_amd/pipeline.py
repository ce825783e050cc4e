"""The skeleton of codon_amd.infer's pipelined loop, on its own: reader threads | the calling thread | one writer thread.
Plain Python (no torch, no library), so tests/test_pipeline_cpu.py runs every path of it -- the failing ones too -- without a GPU."""
from __future__ import annotations

import queue
import threading

_END = object()                 # ends a queue; no stage can return it


def run_pipeline(items, load, step, settle, write, readers=3, name="pipeline"):
    """For every item, in order: load(item) -> loaded in one of `readers` threads (thread k takes items[k::readers], two loaded
    items ahead at the most), step(loaded) -> (to_settle, to_write) on the calling thread, write(to_write) in one writer thread
    (four items behind at the most), and settle(to_settle) on the calling thread once the NEXT item has been stepped -- item
    i - 1 is read back while item i runs -- the last one at the end.  The threads are `{name}_reader{k}` and `{name}_writer`.
    An exception of any stage is raised here, the first one recorded if there are several.  A reader's failure arrives in item
    order, after the items ahead of it have been stepped; for the writer's the calling thread looks once per item and steps no
    further, and a writer that failed keeps emptying its queue so that nothing can block on it.  Readers blocked on a full
    queue are released, and no thread of the pipeline is alive when this returns or raises."""
    items = list(items)
    if not items:
        return
    q_ins = [queue.Queue(maxsize=2) for _ in range(readers)]
    q_out: "queue.Queue" = queue.Queue(maxsize=4)
    errs = []
    stop = threading.Event()

    def reader(k):
        try:
            for item in items[k::readers]:
                if stop.is_set():
                    break
                q_ins[k].put(load(item))
        except BaseException as e:      # noqa: BLE001 -- raised in the calling thread
            errs.append(e)
        finally:
            q_ins[k].put(_END)

    def writer():
        failed = False
        while (w := q_out.get()) is not _END:
            if not failed:              # after a failure: only empty the queue, up to the end mark
                try:
                    write(w)
                except BaseException as e:      # noqa: BLE001
                    failed = True
                    errs.append(e)
                    stop.set()

    trs = [threading.Thread(target=reader, args=(k,), name=f"{name}_reader{k}") for k in range(readers)]
    tw = threading.Thread(target=writer, name=f"{name}_writer")
    for t in trs + [tw]:
        t.start()
    pending = _END
    try:
        for i in range(len(items)):
            if stop.is_set():                       # the writer failed
                break
            loaded = q_ins[i % readers].get()       # the queues in turn: items are consumed in order
            if loaded is _END:                      # that reader failed: the items ahead of its failure have been stepped
                break
            to_settle, to_write = step(loaded)
            q_out.put(to_write)
            if pending is not _END:
                settle(pending)                     # item i - 1, while item i runs
            pending = to_settle
        if pending is not _END:
            settle(pending)
    except BaseException as e:          # noqa: BLE001 -- after the threads have ended, like theirs
        errs.append(e)
    finally:
        stop.set()
        q_out.put(_END)                 # cannot block for good: the writer empties its queue whatever happened
        for t, q in zip(trs, q_ins):    # a reader may be blocked on a full queue
            while t.is_alive():
                try:
                    q.get_nowait()
                except queue.Empty:
                    pass
                t.join(0.02)
        tw.join()
    if errs:
        raise errs[0]

"""HIP-graph replay of the inference forward for launch-bound sizes.

At the reference's own use case (one image per call, test.py:125) the ~95 kernel launches of a forward cost more
than the kernels at small sizes (config 0: 1x128x128).  The forward is a fixed launch sequence with no host
synchronisation and no data-dependent control flow, so it is captured ONCE into a hipGraph (torch.cuda.CUDAGraph:
capture stream, graph-private memory pool) and replayed per call: one launch instead of ~95."""
from __future__ import annotations

import torch


class GraphedCODON:
    def __init__(self, model, example_x: torch.Tensor, example_y: torch.Tensor, warmup: int = 2):
        if not example_x.is_cuda:
            raise RuntimeError("GraphedCODON needs HIP tensors")
        if warmup < 1:
            # the warm-up forward is what packs the weights, allocates the weight guard's pinned flag word and RECORDS the
            # checksum the captured launch compares with; none of that may happen for the first time under capture
            raise ValueError("GraphedCODON: warmup must be >= 1")
        self.model = model.eval()
        # 16-bit images for a model whose activations have that type (the reference script's model.cuda().half() on .half()
        # inputs, test.py:52,122-123) stay 16-bit: the captured forward converts them in its own first launch and its head
        # stores the 16-bit output -- no conversion launches outside the graph
        self.io_dtype = example_x.dtype if (example_x.dtype == example_y.dtype and example_x.dtype != torch.float32 and
                                            example_x.dtype == self.model._act_dtype()) else torch.float32
        self.x = example_x.detach().clone().to(self.io_dtype).contiguous()
        self.y = example_y.detach().clone().to(self.io_dtype).contiguous()
        side = torch.cuda.Stream(device=self.x.device)
        side.wait_stream(torch.cuda.current_stream(self.x.device))
        with torch.no_grad(), torch.cuda.stream(side):
            for _ in range(warmup):                      # packs the weights, warms the allocator
                self.model._forward_impl(self.x, self.y, None, out_dtype=self.io_dtype)
        torch.cuda.current_stream(self.x.device).wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(self.graph):
            self.out = self.model._forward_impl(self.x, self.y, None, out_dtype=self.io_dtype)
        # the captured launches carry raw addresses of the packed weight images (ordinary allocator pool) and of the
        # small fp32 parameters: keep the former alive for the graph's lifetime and remember which weight values
        # they were packed from, so a replay after a weight update is refused instead of silently stale
        self._packed_refs = [v[1] for v in self.model._pack_cache.values()]
        self._tags = self._weight_tags()
        # ... and of the weight guard's workspace, reference slot and host-visible flag word (guards._WeightGuard): the captured
        # checksum launch compares on every replay and reports into THIS flag word, whatever the model's guard does later.
        # The capture's own state comes from the graph's pool and is never cached (guards.PerStream): `captured` hands it over
        g = getattr(self.model, "_wguard", None)
        self._guard_refs = (g.flag, list(g.states.values()) + list(g.captured)) if g is not None else None
        if g is not None:
            g.captured.clear()
        self._flag_np = g.flag_np if g is not None else None
        # ... and of the non-finite input guard (guards._InputGuard): the captured stems store into the model's two pinned host
        # words (only ever zeroed in place, so the captured address stays the live one) and into per-image device words from
        # the graph's pool, which the captured checksum launch (or memset) zeroes on every replay
        ig = self.model.__dict__.get("_iguard")
        self._nf_mode = self.model._nf_mode() if hasattr(self.model, "_nf_mode") else "ignore"
        self._nf_guard = ig
        self._nf_refs = (ig.words, list(ig.captured)) if ig is not None else None
        if ig is not None:
            ig.captured.clear()

    def _weight_tags(self):
        return [(p.data_ptr(), p._version) for p in self.model.parameters()]

    def stale(self, synchronize: bool = False) -> bool:
        """True when a parameter was replaced or modified after capture: autograd-visibly (host-side tags), or through
        `.data` -- the captured forward carries the model's weight-checksum launch (model._WeightGuard), so a replay on
        such weights sets the guard's host-visible flag; with synchronize=True every replay enqueued so far is judged."""
        if self._weight_tags() != self._tags:
            return True
        if synchronize:
            torch.cuda.synchronize(self.x.device)
        if self._flag_np is not None and bool(self._flag_np[0]):
            return True
        try:
            self.model.check_packed(synchronize=False)
        except RuntimeError:
            return True
        return False

    def __call__(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        if x.shape != self.x.shape:
            raise RuntimeError(f"GraphedCODON was captured for {tuple(self.x.shape)}, got {tuple(x.shape)}")
        if self.stale():
            raise RuntimeError("GraphedCODON: the model's parameters changed after capture (visibly, or through `.data`: "
                               "stale packed weights were replayed); build a new GraphedCODON")
        if self._nf_mode == "raise" and self._nf_guard is not None:
            # a replay (or an eager forward of the model) since the last report ran on a non-finite input: one host read per
            # word, no synchronisation -- the offending replay has been enqueued by then, this call raises
            self._nf_guard.report(False, " [GraphedCODON replay]")
        self.x.copy_(x)
        self.y.copy_(y)
        self.graph.replay()
        return self.out.clone()

"""Particle-sharded SVGD iteration over the GPUs of one node (one process per GPU,
`torch.distributed`, backend "nccl" = RCCL over xGMI on ROCm; "gloo" in the CPU tests).

The reference has no distributed code; this is new design for the path's
natural sharding: N^2/2 independent pair solves followed by one reduction over partners.

    rank r owns particle rows [r*N/G, (r+1)*N/G)
    1. all-gather   X and score shards (2*N*T*d*4 B; 3.7 MB at N=1024,T=64,d=7) into two contiguous operands, issued as
                    ONE grouped RCCL operation (ncclGroupStart / ncclGroupEnd through torch's coalescing manager: a single
                    launch on this latency-bound path); gloo, which has no grouped form, issues them one after the other
    2. compute      the unordered pairs {i <= j} whose row tile (ops.sym_tile_rows(T, d) rows: 4 for T <= 64 with
                    d > 8, else 8) has index r, r + G, ... or is the mirror image ntile-1-t of such a tile
                    (FOLDED ownership: in the upper triangle tile t holds N - t*rows columns, so a tile and
                    its mirror image always hold the same number of pairs and every rank gets the same
                    share; cyclic ownership alone gives the first rank 5.4 % more than the mean at N=1024,
                    G=8), on the gathered X:  K_partial [N,N], grad_partial [N,T,d]
                    LONG ROUTE (launches the fused kernels refuse: long paths, refined grids past the LDS; and any shape
                    with long_partial=True): the same ownership, folded or cyclic, on row tiles of
                    ops.gram_long_partial_tiles(...)[0] rows, solved by ops.gram_long_sym_partial at the step's dyadic
                    order and static kernel -- each unordered pair once across the node there too
                    v_partial = -((K_partial @ score - grad_partial)/N)   (linear in the partials)
    3. reduce-scatter(sum) v_partial -> this rank's rows of v;  X_shard <- X_shard - lr * v  (one launch)
                    With a mask, update="adagrad" or update="adam" the update is ops.svgd_update on the rank's rows instead
                    (one launch, the fused single-GPU launches' device function): mask, Adagrad and Adam are not linear in
                    the partials, so they run behind the reduce-scatter, on state this rank keeps for its own rows.
All per-step buffers (gathered operands, partials, velocity, optimizer state) are allocated once and reused.
K itself stays distributed (each rank keeps its partial; `gather_gram` sums it on demand).

Both collectives are latency-bound at these sizes (a 229 KB shard per peer over a dedicated xGMI
link), so nothing is bucketed or pipelined; the pair solve dominates.
"""
from __future__ import annotations

from typing import Callable, Optional, Tuple

import torch
import torch.distributed as dist

from . import _lib, ops


def _world(group=None) -> Tuple[int, int]:
    return dist.get_rank(group), dist.get_world_size(group)


def shard_rows(N: int, rank: int, world: int) -> Tuple[int, int]:
    if N % world != 0:
        raise ValueError(f"particle count {N} must be divisible by the number of ranks {world}")
    per = N // world
    return rank * per, (rank + 1) * per


def all_gather_rows(shard: torch.Tensor, group=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[N/G, ...] -> [N, ...] (rank order)."""
    world = dist.get_world_size(group)
    if out is None:
        out = torch.empty((shard.shape[0] * world,) + tuple(shard.shape[1:]), dtype=shard.dtype, device=shard.device)
    dist.all_gather_into_tensor(out, shard.contiguous(), group=group)
    return out


def all_gather_rows_pair(a: torch.Tensor, b: torch.Tensor, out_a: torch.Tensor, out_b: torch.Tensor, group=None) -> bool:
    """Two all-gathers (same shard shape) into their own contiguous outputs as one grouped collective where the backend has
    one (RCCL: ncclGroupStart / ncclGroupEnd, a single launch); otherwise back to back.  Returns whether the grouped form ran."""
    a, b = a.contiguous(), b.contiguous()
    if dist.get_backend(group) == "nccl" and hasattr(dist, "_coalescing_manager"):
        try:
            with dist._coalescing_manager(group=group, device=a.device, async_ops=False):
                dist.all_gather_into_tensor(out_a, a, group=group)
                dist.all_gather_into_tensor(out_b, b, group=group)
            return True
        except (RuntimeError, TypeError, NotImplementedError):  # a torch build without the grouped form for this op
            pass
    dist.all_gather_into_tensor(out_a, a, group=group)
    dist.all_gather_into_tensor(out_b, b, group=group)
    return False


def reduce_scatter_rows(full: torch.Tensor, group=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """sum over ranks of [N, ...] -> this rank's [N/G, ...] rows."""
    world = dist.get_world_size(group)
    if out is None:
        out = torch.empty((full.shape[0] // world,) + tuple(full.shape[1:]), dtype=full.dtype, device=full.device)
    if dist.get_backend(group) == "gloo":  # gloo has no reduce_scatter: all-reduce then slice (tests only)
        tmp = full.contiguous().clone()
        dist.all_reduce(tmp, group=group)
        r = dist.get_rank(group)
        out.copy_(tmp[r * out.shape[0]:(r + 1) * out.shape[0]])
        return out
    dist.reduce_scatter_tensor(out, full.contiguous(), group=group)
    return out


class _PhaseClock:
    """Per-phase timing of one sharded step: HIP events on the current stream (the collectives and the
    library's launches are all enqueued there), host clocks for CPU tensors (gloo rehearsal)."""

    def __init__(self, device: torch.device):
        self.gpu = device.type == "cuda"
        self.names = []
        self.marks = [self._now()]

    def _now(self):
        if self.gpu:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            return ev
        import time

        return time.perf_counter()

    def __call__(self, name: str) -> None:
        self.names.append(name)
        self.marks.append(self._now())

    def result(self) -> dict:
        if self.gpu:
            torch.cuda.synchronize()
            return {n: self.marks[k].elapsed_time(self.marks[k + 1]) for k, n in enumerate(self.names)}
        return {n: (self.marks[k + 1] - self.marks[k]) * 1e3 for k, n in enumerate(self.names)}


class ShardedSigSVGD:
    """One SVGD iteration with particles sharded across ranks.

    partial_fn(X_full, inv_h, tile_offset, tile_stride[, out=, fold=]) -> (K_partial, grad_partial) defaults to the
    HIP library's symmetric partial solve with folded tile ownership; phi_fn(K, score, grad_k) -> v to the MFMA velocity
    kernel.  (The CPU tests substitute oracle-backed callables to exercise the sharding algebra under gloo.)

    dyadic_order / static_kind: the step's refinement and built-in static kernel.  The route of a step, in this order:
    rowwise=True -> (own rows) x (all columns); the fused partial solve where it takes the shape (order 0, RBF, T <= 128,
    d <= 16); the row-wise solve where the fused kernels take the launch, and always with a caller's rows_fn (unless a
    long_partial_fn is given too: a caller's row solver keeps the launches it got before); else the long partial solve
    long_partial_fn(X_full, inv_h, tile_offset, tile_stride, dyadic_order=, static_kind=, out=, fold=) -> (K_partial,
    grad_partial), by default `ops.gram_long_sym_partial`; else the row-wise call's own error.  static_kind 2, 3, 6 and 7 (IMQ,
    rational quadratic, Matern-3/2 and -5/2: the fp64 coverage kernel and the long route, never the fused partial solve): their
    row-wise step
    takes `ops.gram_long_fwd_bwd` at a shape only the long route takes.  long_partial=True sends every
    shape the long partial takes to it (each pair once also at 129 <= T <= 190), long_partial=False never uses it.
    `last_route` names the last step's route ("partial", "rowwise" or "long_partial"); `route(X_shard)` answers it without a step.
    fp32_sweeps=True with static_kind 2 or 3 at order 0: the fused partial solve takes the step at
    3 <= T <= 64, d <= 16 (`ops.gram_sym_partial(..., static_kind=, fp32_sweeps=True)`: the register-resident kernel, each
    unordered pair once, K within 1e-5 per entry instead of fp64 results), and the row-wise solve passes the flag too.  With RBF
    at order 0 it sends the row-wise step of 17 <= d <= 32 channels, 3 <= T <= 64, to the register-resident kernel (section 5.25;
    the partial solve stops at 16 channels); with any other kind it changes nothing.

    update: "manual" (X - lr * v, the reference's optimizer=None), "adagrad" (its adaptive_gradient=True) or "adam"
    (torch.optim.Adam with `betas`, `eps`; lr is its learning rate); mask: multiplies the velocity, broadcastable to the
    shard [n, T, d] (TrajectorySVGD's gradient_mask, this rank's rows of it).  All three routes end in one call
    update_fn(v_rows, X_shard, lr, mask=, adagrad_state=, adam=, want_v=False) -> (None, X_new), by default
    `ops.svgd_update` (the CPU tests pass a torch restatement); update="manual" without a mask keeps the plain torch.add.
    That call computes in fp32 (state and arithmetic, as the fused single-GPU launches do) and the result is cast back to
    the shard's dtype: an fp64 shard keeps its dtype but not fp64 updates, unlike on the plain path.  The state covers
    this rank's rows, is zeroed once per shard shape and is saved / restored with `state_dict()` / `load_state_dict()`.
    `last_v_rows` is the last step's reduced velocity on this rank's rows BEFORE mask and update; on the partial routes it
    ALIASES the step's preallocated buffer, which the next step() overwrites (clone to keep it)."""

    def __init__(self, inv_h: float, lr: float, group=None, partial_fn: Optional[Callable] = None,
                 phi_fn: Optional[Callable] = None, rows_fn: Optional[Callable] = None, rowwise: bool = False,
                 fold: bool = True, dyadic_order: int = 0, static_kind: int = _lib.STATIC_RBF,
                 long_partial: Optional[bool] = None, long_partial_fn: Optional[Callable] = None,
                 update: str = "manual", betas=(0.9, 0.999), eps: float = 1e-8, mask=None,
                 update_fn: Optional[Callable] = None, fp32_sweeps: bool = False):
        if update not in ("manual", "adagrad", "adam"):
            raise ValueError(f'update must be "manual", "adagrad" or "adam", got {update!r}')
        self.update = update
        self.betas = (float(betas[0]), float(betas[1]))
        self.eps = float(eps)
        self.mask = mask
        self.update_fn = update_fn or ops.svgd_update
        self.last_v_rows = None  # ALIASES the step's buffer, like last_K_partial
        self._steps = 0          # updates done (what state_dict() saves as "step")
        self._loaded = None      # a load_state_dict() waiting for the first step's buffers
        self.inv_h = float(inv_h)
        self.lr = float(lr)
        self.group = group
        self.fold = bool(fold)
        self.dyadic_order = int(dyadic_order)
        self.static_kind = int(static_kind)
        self.fp32_sweeps = bool(fp32_sweeps)
        # the IMQ / rational-quadratic step on the fp32-sweep kernels: the keyword goes to `ops` only where it is set
        self._fast_radial = self.fp32_sweeps and self.dyadic_order == 0 and self.static_kind in (_lib.STATIC_IMQ, _lib.STATIC_RQ)
        self._fp32_kw = {"fp32_sweeps": True} if self.fp32_sweeps else {}
        self.long_partial = None if long_partial is None else bool(long_partial)
        self.long_partial_fn = long_partial_fn or ops.gram_long_sym_partial
        self._long_fold = bool(fold)  # (the 4-argument fallback below concerns partial_fn only)
        self.last_route = None
        self._routes = {}
        if partial_fn is None and self._fast_radial:
            partial_fn = lambda X, inv_h, off, stride, out=None, fold=False: ops.gram_sym_partial(
                X, inv_h, off, stride, static_kind=self.static_kind, out=out, fold=fold, fp32_sweeps=True)
        self.partial_fn = partial_fn or ops.gram_sym_partial
        # `out=` / `fold=` are passed only to callables that take them (the 4-argument contract of rounds 1-2 still works;
        # such a callable owns cyclic tiles and allocates its results)
        import inspect

        try:
            params = inspect.signature(self.partial_fn).parameters
            self._partial_kwargs = ("out" in params and "fold" in params) or any(
                q.kind is inspect.Parameter.VAR_KEYWORD for q in params.values())
        except (TypeError, ValueError):
            self._partial_kwargs = True
        if not self._partial_kwargs and self.fold and partial_fn is not None:
            self.fold = False  # (cyclic ownership is what a 4-argument callable implements)
        self.phi_fn = phi_fn or (lambda K, s, gk: ops.svgd_phi(K, s, gk))
        # the long route is taken by itself only in place of the library's own row-wise solve: a caller's rows_fn keeps the
        # launches it got before, unless the caller asks for the long partial (long_partial=True or a long_partial_fn)
        self._auto_long = rows_fn is None or long_partial_fn is not None
        if rows_fn is None and self.static_kind in (_lib.STATIC_IMQ, _lib.STATIC_RQ, _lib.STATIC_MATERN32, _lib.STATIC_MATERN52):
            rows_fn = self._rows_fused_or_long
        elif rows_fn is None and (self.dyadic_order != 0 or self.static_kind != _lib.STATIC_RBF):
            rows_fn = lambda Xs, Xf, inv_h: ops.gram_fwd_bwd(Xs, Xf, inv_h, self.dyadic_order, self.static_kind, **self._fp32_kw)
        # (RBF at order 0: the flag changes a row-wise launch of 17 to 32 channels only)
        self.rows_fn = rows_fn or (lambda Xs, Xf, inv_h: ops.gram_fwd_bwd(Xs, Xf, inv_h, **self._fp32_kw))
        self.rowwise = bool(rowwise)
        self.last_K_partial = None  # ALIASES the step's preallocated buffer: the next step() overwrites it (clone to keep it)
        self.last_K_rows = None
        self.phase_ms = None  # filled by step(profile=True): milliseconds per phase on this rank
        self.last_gather_grouped = None  # whether the last step's two all-gathers went out as one grouped collective
        self._buf = {}        # per-step buffers, allocated once per (shape, dtype, device)

    def _buffers(self, X_shard: torch.Tensor, world: int):
        key = (tuple(X_shard.shape), X_shard.dtype, X_shard.device, world)
        b = self._buf.get(key)
        if b is None:
            n, T, d = X_shard.shape
            N, dev, dt = n * world, X_shard.device, X_shard.dtype
            b = {
                "X_full": torch.empty((N, T, d), dtype=dt, device=dev),
                "s_full": torch.empty((N, T, d), dtype=dt, device=dev),
                "K_partial": torch.empty((N, N), dtype=dt, device=dev),
                "grad_partial": torch.empty((N, T, d), dtype=torch.float64, device=dev),
                "v_rows": torch.empty((n, T, d), dtype=dt, device=dev),
            }
            # the update's operands for this rank's rows: the mask spelled out once, the optimizer state zeroed once
            if self.mask is not None:
                b["mask"] = torch.broadcast_to(torch.as_tensor(self.mask, dtype=torch.float32, device=dev),
                                               (n, T, d)).contiguous()
            if self.update == "adagrad":
                b["adagrad"] = torch.zeros((n, T * d), dtype=torch.float32, device=dev)
            elif self.update == "adam":
                b["adam"] = ops.AdamState(X_shard, self.betas, self.eps)
            if self._buf:
                self._steps = 0  # a new shape releases the old buffers and the optimizer state: the count starts again
            self._buf = {key: b}  # one shape at a time
            if self._loaded is not None:
                self._adopt(b, self._loaded)
                self._loaded = None
        return b

    def _state_tensors(self, b) -> dict:
        if self.update == "adagrad":
            return {"adagrad": b["adagrad"]}
        if self.update == "adam":
            return {"exp_avg": b["adam"].exp_avg, "exp_avg_sq": b["adam"].exp_avg_sq}
        return {}

    def state_dict(self) -> dict:
        """The optimizer state of THIS RANK'S rows (every rank saves its own): the mode, the number of updates done, the
        rank and world size it belongs to, and clones of `adagrad` [n, T*d] or `exp_avg` / `exp_avg_sq` [n, T*d]."""
        rank, world = _world(self.group)
        sd = {"update": self.update, "step": self._steps, "rank": rank, "world_size": world}
        if self._loaded is not None:  # loaded and not stepped since
            sd.update({k: t.clone() for k, t in self._loaded.items() if isinstance(t, torch.Tensor)})
        elif self._buf:
            sd.update({k: t.clone() for k, t in self._state_tensors(next(iter(self._buf.values()))).items()})
        return sd

    def load_state_dict(self, sd: dict) -> None:
        """Restores `state_dict()` of the same rank under the same world size and mode (ValueError otherwise: a saved state
        is not resharded); the tensors are copied, onto the particles' device at the latest with the next step."""
        rank, world = _world(self.group)
        if sd["update"] != self.update:
            raise ValueError(f'state of update="{sd["update"]}" loaded into update="{self.update}"')
        if int(sd["world_size"]) != world or int(sd["rank"]) != rank:
            raise ValueError(f'state of rank {sd["rank"]} of {sd["world_size"]} loaded into rank {rank} of {world}')
        want = {"manual": set(), "adagrad": {"adagrad"}, "adam": {"exp_avg", "exp_avg_sq"}}[self.update]
        loaded = {k: sd[k].detach().clone() for k in want if k in sd}
        if set(loaded) != want and (loaded or int(sd["step"]) > 0):
            raise ValueError(f'update="{self.update}" after {sd["step"]} steps needs {sorted(want)}, got {sorted(loaded)}')
        self._steps = int(sd["step"])
        self._loaded = None
        if not loaded:  # a manual step has no tensors, nor has a state saved before the first step: zeroed state
            for b in self._buf.values():  # (in place: the step's other buffers stay)
                for t in self._state_tensors(b).values():
                    t.zero_()
                if self.update == "adam":
                    b["adam"].step.zero_()
                    b["adam"].t_host = 0
            return
        loaded["step"] = self._steps
        if self._buf:
            self._adopt(next(iter(self._buf.values())), loaded)
        else:
            self._loaded = loaded

    def _adopt(self, b, loaded) -> None:
        for k, dst in self._state_tensors(b).items():
            if tuple(loaded[k].shape) != tuple(dst.shape):
                raise ValueError(f"saved {k} {tuple(loaded[k].shape)} does not fit this rank's rows {tuple(dst.shape)}")
            dst.copy_(loaded[k])
        if self.update == "adam":
            b["adam"].step.fill_(int(loaded["step"]))
            b["adam"].t_host = int(loaded["step"])

    def _apply(self, X_shard, v_rows, buf, rowwise: bool = False):
        """The one update of every route, on this rank's rows of the reduced velocity (which `last_v_rows` keeps, untouched)."""
        self.last_v_rows = v_rows
        if self.update == "manual" and self.mask is None:  # the plain step, as it always ran
            out = X_shard - self.lr * v_rows if rowwise else torch.add(X_shard, v_rows, alpha=-self.lr)  # one launch
        else:  # fp32 arithmetic whatever the shard's dtype (the kernel's; the state is fp32), returned in the shard's dtype
            _, X_new = self.update_fn(v_rows, X_shard, self.lr, mask=buf.get("mask"), adagrad_state=buf.get("adagrad"),
                                      adam=buf.get("adam"), want_v=False)
            out = X_new.to(X_shard.dtype)
        self._steps += 1  # (behind the update: a call that raised has changed neither the state nor the count)
        return out

    def step(self, X_shard: torch.Tensor, score_shard: torch.Tensor, profile: bool = False) -> torch.Tensor:
        """Returns the updated shard: X_shard - lr * v_rows, or what the chosen update rule makes of v_rows (a new tensor;
        the step's internal buffers are reused by the next call).  profile=True brackets the phases with events on the
        current stream (device tensors) or host clocks (CPU rehearsal) and leaves the per-phase milliseconds in `self.phase_ms`; it synchronises, so never use it in a
        timed loop."""
        rank, world = _world(self.group)
        mark = _PhaseClock(X_shard.device) if profile else None
        buf = self._buffers(X_shard, world)
        # one grouped collective into preallocated, contiguous operands (no stack / split copies)
        X_full, s_full = buf["X_full"], buf["s_full"]
        self.last_gather_grouped = all_gather_rows_pair(X_shard, score_shard.to(X_shard.dtype), X_full, s_full, self.group)
        if mark:
            mark("all_gather")
        route = self.last_route = self._route(X_shard.shape[0], X_full, world)
        if route == "rowwise":
            out = self._step_rowwise(X_shard, X_full, s_full, buf)
            if mark:
                mark("rowwise_solve_and_update")
                self.phase_ms = mark.result()
            return out
        if route == "long_partial":
            Kp, gp = self.long_partial_fn(X_full, self.inv_h, rank, world, dyadic_order=self.dyadic_order,
                                          static_kind=self.static_kind, out=(buf["K_partial"], buf["grad_partial"]),
                                          fold=self._long_fold)
        elif self._partial_kwargs:  # (a user callable written to the 4-argument contract gets no preallocated outputs)
            Kp, gp = self.partial_fn(X_full, self.inv_h, rank, world, out=(buf["K_partial"], buf["grad_partial"]),
                                     fold=self.fold)
        else:
            Kp, gp = self.partial_fn(X_full, self.inv_h, rank, world)
        if mark:
            mark("partial_solve")
        self.last_K_partial = Kp
        v_part = self.phi_fn(Kp, s_full, gp.to(s_full.dtype))  # -((Kp @ s - gp)/N), linear in (Kp, gp)
        if mark:
            mark("velocity")
        v_rows = reduce_scatter_rows(v_part.reshape(X_full.shape), self.group, out=buf["v_rows"])
        if mark:
            mark("reduce_scatter")
        out = self._apply(X_shard, v_rows, buf)
        if mark:
            mark("update")
            self.phase_ms = mark.result()
        return out

    def route(self, X_shard: torch.Tensor, world: Optional[int] = None) -> str:
        """The route `step` takes for a shard of this shape ("partial", "rowwise" or "long_partial"), from host-only queries of
        the library; world: the number of ranks (default: the group's)."""
        if world is None:
            world = _world(self.group)[1]
        n, T, d = X_shard.shape
        return self._route(n, torch.empty((n * world, T, d), dtype=X_shard.dtype, device="meta"), world)

    def _route(self, n_own: int, X_full, world: int) -> str:
        """"partial" (fused), "rowwise" or "long_partial" for this step's shape; see the class docstring for the order"""
        N, T, d = X_full.shape
        if self.rowwise:
            return "rowwise"
        key = (n_own, N, T, d, world)
        if key not in self._routes:  # (host-only queries of the library, asked once per shape)
            self._routes[key] = self._route_of(n_own, X_full, world)
        return self._routes[key]

    def _route_of(self, n_own: int, X_full, world: int) -> str:
        N, T, d = X_full.shape
        takes_long = lambda: ops.gram_long_partial_takes(N, T, d, self.dyadic_order, self.static_kind, world)
        if self.long_partial and takes_long():
            return "long_partial"
        if self.dyadic_order == 0 and self.static_kind == _lib.STATIC_RBF and self._partial_supported(X_full):
            return "partial"
        # (IMQ / rational quadratic with fp32_sweeps: the register-resident kernel's lengths only, the quadrant kernel is RBF's)
        if self._fast_radial and 3 <= T <= 64 and self._partial_supported(X_full):
            return "partial"
        if self.long_partial is None and self._auto_long \
                and not ops.gram_takes(n_own, N, T, d, self.dyadic_order, self.static_kind, **self._fp32_kw) and takes_long():
            return "long_partial"
        return "rowwise"

    def _rows_fused_or_long(self, Xs, Xf, inv_h):
        """The library's row solver of the IMQ, rational-quadratic and Matern kernels: the fused launch where the coverage kernel
        takes the rows' shape, else the long route's ordered launch (a row-wise step at a shape only the long route takes:
        rowwise=True, long_partial=False)."""
        n, T, d = Xs.shape
        if ops.gram_takes(n, Xf.shape[0], T, d, self.dyadic_order, self.static_kind, **self._fp32_kw):
            return ops.gram_fwd_bwd(Xs, Xf, inv_h, self.dyadic_order, self.static_kind, **self._fp32_kw)
        return ops.gram_long_fwd_bwd(Xs, Xf, inv_h, self.dyadic_order, self.static_kind)

    @staticmethod
    def _partial_supported(X_full) -> bool:
        """shapes the symmetric partial solve takes (the library's routing rule)"""
        return ops.sym_tile_rows(X_full.shape[1], X_full.shape[2]) > 0

    def _step_rowwise(self, X_shard, X_full, s_full, buf):
        """Fallback for shapes outside the symmetric partial solve (e.g. T > 128): each rank solves
        the ordered pairs (own rows) x (all columns), so its rows of K, grad_k and v are complete
        locally and no reduce-scatter is needed -- at twice the pair solves."""
        K_rows, g_rows = self.rows_fn(X_shard, X_full, self.inv_h)
        self.last_K_partial = None
        self.last_K_rows = K_rows
        n_all = X_full.shape[0]
        v_rows = -((K_rows.to(s_full.dtype) @ s_full.flatten(1) - g_rows.flatten(1).to(s_full.dtype)) / n_all)
        return self._apply(X_shard, v_rows.reshape(X_shard.shape), buf, rowwise=True)

    def gather_gram(self) -> torch.Tensor:
        """Full K (sum of the partials), on demand -- the per-iteration path never needs it."""
        if self.last_K_partial is None:  # row-wise step: rows are complete, just gather them
            return all_gather_rows(self.last_K_rows, self.group)
        K = self.last_K_partial.clone()
        dist.all_reduce(K, group=self.group)
        return K

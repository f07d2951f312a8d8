"""Basis base class (drop-in for src/projected_langevin_sampling/basis/base.py:7-193)."""
from __future__ import annotations

from abc import ABC, abstractmethod
from typing import Optional

import torch

from .. import _lib as L
from ..kernel import _dev

#: default cap of the per-step G-chunk workspace (bytes); bigger = fewer, larger GEMM launches
DEFAULT_WORKSPACE_BYTES = 2 << 30


#: bit pattern a consumer writes into a slot of BlockSpec.energy_sums before it queues the launch that fills it: a quiet NaN
#: with a payload no computation produces (a diverged run's NaN / inf energies are ordinary values next to it)
UNWRITTEN_ENERGY_BITS = 0x7FF8DEADBEEF0001


class NoiseSpec:
    """How one Langevin step gets its noise.
    injected: a (M, J) device tensor used as-is (parity runs inject the oracle's noise);
    philox:   libplship's counter-based stream keyed by (seed, step, row, j_offset + column)."""

    def __init__(self, injected: torch.Tensor | None = None, seed: int | None = None, step: int = 0, j_offset: int = 0,
                 none: bool = False, step_base: torch.Tensor | None = None):
        self.injected, self.seed, self.step, self.j_offset, self.none = injected, seed, step, j_offset, none
        #: optional device int64 scalar added to ``step`` at kernel run time (lets a captured graph draw fresh noise)
        self.step_base = step_base

    def desc(self) -> L.NoiseDesc:
        d = L.NoiseDesc()
        if self.none:
            d.kind = L.NOISE_NONE
        elif self.injected is not None:
            xi = L.require_gpu_tensor(self.injected, "noise", promote=True)
            assert xi.stride(-1) == 1
            d.kind, d.xi, d.ldxi = L.NOISE_INJECTED, xi.data_ptr(), L.ld(xi)
        else:
            d.kind, d.seed, d.step, d.j_offset = L.NOISE_PHILOX, int(self.seed) & (2**64 - 1), int(self.step), int(self.j_offset)
            if self.step_base is not None:
                assert self.step_base.device.type == "cuda" and self.step_base.dtype == torch.int64 and self.step_base.numel() == 1
                d.step_base = self.step_base.data_ptr()
        return d


class BlockSpec:
    """One step size per column block of the particle matrix (pls_block_desc): the S candidates of a step-size search
    run as S blocks of ``block_cols`` columns.  ``eta`` is a device float64 vector, one entry per block; writing 0
    freezes a block."""

    def __init__(self, block_cols: int, eta: torch.Tensor, energy_sums: int | None = None,
                 energy_sync: torch.Tensor | None = None, energy_partials: torch.Tensor | None = None,
                 energy_partials_prev: torch.Tensor | None = None, energy_prev: torch.Tensor | None = None,
                 energy_sums_prev: int | None = None, energy_flush: bool = False, step_sync: torch.Tensor | None = None,
                 energy_sums16: int | None = None):
        """``energy_sums`` (optional): raw address (device, or pinned host memory) of cdiv(J, 256) doubles that receive the
        256-column chunk sums of the per-particle energies from the launch that finishes the step's energy by-product
        (Gaussian/identity fast paths; see pls_block_desc)."""
        assert block_cols > 0
        L.require_gpu_tensor(eta, "eta")
        assert eta.dim() == 1 and eta.is_contiguous()
        self.block_cols, self.eta, self.energy_sums = int(block_cols), eta, energy_sums
        #: optional: device int32 counters, one per 256 columns, zeroed once by the owner (pls_block_desc.energy_sync): the step
        #: launch then finishes the energies itself and leaves the counters zero
        if energy_sync is not None:
            assert energy_sync.device.type == "cuda" and energy_sync.dtype == torch.int32 and energy_sync.is_contiguous()
        self.energy_sync = energy_sync
        #: LAGGED energies (pls_block_desc.energy_partials ...): this launch leaves its partial rows in ``energy_partials``
        #: and finishes the previous launch's (``energy_partials_prev``) into ``energy_prev`` (J device doubles) and, optionally,
        #: ``energy_sums_prev`` (raw address of cdiv(J, 256) doubles, device or pinned host memory); ``energy_flush``: no
        #: step, only that finish (OrthonormalBasis.flush_energies, BoundStep.flush)
        for t in (energy_partials, energy_partials_prev, energy_prev):
            if t is not None:
                L.require_gpu_tensor(t, "energy buffer")
                assert t.is_contiguous()
        self.energy_partials, self.energy_partials_prev, self.energy_prev = energy_partials, energy_partials_prev, energy_prev
        self.energy_sums_prev, self.energy_flush = energy_sums_prev, bool(energy_flush)
        #: optional: device int32 counters (pls_step_sync_words(J) of them), zeroed once by the owner: the one-launch small-rank
        #: step (pls_block_desc.step_sync) meets through them and leaves them zero
        if step_sync is not None:
            assert step_sync.device.type == "cuda" and step_sync.dtype == torch.int32 and step_sync.is_contiguous()
        self.step_sync = step_sync
        #: optional: raw address (device, or pinned host memory) of cdiv(J, 16) doubles that receive the sums of the energies over
        #: each block of 16 columns (pls_block_desc.energy_sums16)
        self.energy_sums16 = energy_sums16

    def desc(self) -> L.BlockDesc:
        d = L.BlockDesc()
        d.block_cols, d.eta = self.block_cols, self.eta.data_ptr()
        d.energy_sums = self.energy_sums
        d.energy_sync = None if self.energy_sync is None else self.energy_sync.data_ptr()
        d.energy_partials = None if self.energy_partials is None else self.energy_partials.data_ptr()
        d.energy_partials_prev = None if self.energy_partials_prev is None else self.energy_partials_prev.data_ptr()
        d.energy_prev = None if self.energy_prev is None else self.energy_prev.data_ptr()
        d.energy_sums_prev = self.energy_sums_prev
        d.energy_flush = 1 if self.energy_flush else 0
        d.step_sync = None if self.step_sync is None else self.step_sync.data_ptr()
        d.energy_sums16 = self.energy_sums16
        return d


class StepRoute:
    """A basis' answer to "how does one step of this cost over ``j`` particle columns run" (PLSBasis._route): the C entry --
    ``entry`` takes the step size as a double, ``blocks_entry`` a pls_block_desc (after ``blocks_head``) --, the arguments
    in front of the particles (the descriptor, Gaussian constants prepared, the cost descriptor and the targets) and behind
    the output mode, the workspace bytes it asks for, and whether it is the one-launch small-rank step, which meets through
    zeroed arrival counters (pls_block_desc.step_sync).  ``holds``: what the descriptor points into.  ``sums`` / ``lagged``:
    the step can leave the 256-column chunk sums of its energy by-product / finish them one launch later."""

    __slots__ = ("entry", "blocks_entry", "fn", "fn_blocks", "head", "tail", "blocks_head", "ws_bytes", "ws_for_energy_only",
                 "holds", "one_launch", "sums", "lagged")

    def __init__(self, entry, blocks_entry, head, tail, ws_bytes, holds, one_launch=False, sums=False, lagged=False,
                 ws_for_energy_only=False, blocks_head=()):
        lib = L.load()
        self.entry, self.blocks_entry = entry, blocks_entry
        self.fn = None if entry is None else getattr(lib, entry)
        self.fn_blocks = getattr(lib, blocks_entry)
        self.head, self.tail, self.blocks_head = head, tail, blocks_head
        self.ws_bytes, self.ws_for_energy_only, self.holds = int(ws_bytes), ws_for_energy_only, holds
        self.one_launch, self.sums, self.lagged = one_launch, sums, lagged

    def workspace_bytes(self, with_energy: bool) -> int:
        return 0 if self.ws_for_energy_only and not with_energy else self.ws_bytes

    def call(self, bd, u_ptr, ldu, j, step_size, nd, out_ptr, ldo, mode, energy_ptr, ws_ptr, ws_bytes, stream) -> int:
        mid = (step_size,) if bd is None else (*self.blocks_head, bd)
        fn = self.fn if bd is None else self.fn_blocks
        return fn(*self.head, u_ptr, ldu, j, *mid, nd, out_ptr, ldo, mode, *self.tail, energy_ptr, ws_ptr, ws_bytes, stream)


class BoundStep:
    """One step call bound once for a loop that makes it thousands of times (PLSBasis._bind_step): at the reference's own
    problem sizes a step is a 5-10 us kernel, and building the call afresh (descriptors, workspace, counters: ~10-20 us of
    Python) is what an iteration would cost.  The object OWNS every tensor whose address sits in its descriptors -- the
    workspace, the step-size word, the arrival counters, the lagged partial rows, and (``route.holds``) the basis constants --,
    so nothing it launches with can be freed or replaced under it.

    ``form`` -- what a launch does with the energies of its input particles:
      "none"    no energies (the drop-in step);
      "lagged"  leaves their partial rows; the NEXT launch finishes them into its ``energy`` / ``slot`` (reports_previous)
                at its start, under the landing of its first operand rows -- the reduction's serial tail (4-5 us) leaves the
                critical path; the last launch's rows take a small launch of their own (flush);
      "sums"    the 256-column chunk sums into ``slot``, finished by the step launch itself (pls_block_desc.energy_sync:
                ONE launch per iteration, no separate finishing or mean launch);
      "sums16"  the 16-column sums into ``slot`` (the one-launch small-rank step);
      "means"   the per-particle energies into ``energy``, then their mean into ``slot`` (pls_block_means).
    A launch: bound.launch(u_ptr, ldu, out_ptr, ldo, noise, energy_ptr, slot_ptr), ``noise`` the Philox key, or the (M, J)
    device noise matrix when bound with ``injected``; ``slot``: ``slot_doubles`` doubles, device or pinned host memory.
    (``launch`` is a closure over what it needs: at these sizes an attribute lookup per argument is a measurable share.)"""

    def __init__(self, basis, route: StepRoute, state: torch.Tensor, step_size: float, form: str, injected: bool = False,
                 new_state: bool = True):
        assert form in ("none", "lagged", "sums", "sums16", "means")
        lib, dev = L.load(), state.device
        j = self.j = state.shape[1]
        self.route, self.form, self.injected, self.step_size = route, form, bool(injected), float(step_size)
        self.reports_previous = form == "lagged"
        self.slot_doubles = (0 if form == "none" else 1 if form == "means" else (j + 15) // 16 if form == "sums16"
                             else (j + 255) // 256)
        ws_bytes = route.workspace_bytes(form not in ("none", "lagged"))
        self.workspace = torch.empty((ws_bytes + 7) // 8, dtype=torch.float64, device=dev) if ws_bytes else None
        self.eta = step_sync = energy_sync = bd = None
        self.partials = part = ()
        if form != "means" and (form != "none" or route.one_launch):
            self.eta = torch.full((1,), self.step_size, dtype=torch.float64, device=dev)
            bd = L.BlockDesc()
            bd.block_cols, bd.eta = j, self.eta.data_ptr()
            if route.one_launch:
                step_sync = torch.zeros(max(int(lib.pls_step_sync_words(j)), 1), dtype=torch.int32, device=dev)
                bd.step_sync = step_sync.data_ptr()
            if form == "sums":
                energy_sync = torch.zeros(self.slot_doubles, dtype=torch.int32, device=dev)
                bd.energy_sync = energy_sync.data_ptr()
            if form == "lagged":
                pbytes = basis.energy_partial_rows_bytes(j)
                self.partials = tuple(torch.empty((pbytes + 7) // 8, dtype=torch.float64, device=dev) for _ in range(2))
                part = tuple(p.data_ptr() for p in self.partials)
        self.blocks, self.step_sync, self.energy_sync, self._part_ptr = bd, step_sync, energy_sync, part
        nd = L.NoiseDesc()
        if injected:
            nd.kind = L.NOISE_INJECTED
        else:
            nd.kind, nd.step, nd.j_offset = L.NOISE_PHILOX, 0, int(basis.j_offset)
        fn = route.fn if bd is None else route.fn_blocks
        mid = (self.step_size,) if bd is None else (*route.blocks_head, bd)
        mode = L.OUT_NEW_STATE if new_state else L.OUT_DELTA
        ws_ptr, stream, means = L.ptr(self.workspace), L.stream_ptr(), lib.pls_block_means
        # the C entry's argument list, built once: a launch stores its particle, output and energy addresses into it
        args = [*route.head, None, None, j, *mid, nd, None, None, mode, *route.tail, None, ws_ptr, ws_bytes, stream]
        iu = len(route.head)
        io = iu + 4 + len(mid)
        ie = io + 3 + len(route.tail)
        launches = self._launches = [0]  # (lagged: which partial-row buffer a launch leaves its rows in)
        entry = route.entry if bd is None else route.blocks_entry
        self._stream, self.workspace_ptr = stream, ws_ptr

        def failed(rc: int) -> None:
            # stale arrival counters would make every later launch wrong: zero them before the error goes up
            for t in (step_sync, energy_sync):
                if t is not None:
                    t.zero_()
            L.check(rc, entry)

        def launch(u_ptr, ldu, out_ptr, ldo, noise, energy_ptr=None, slot_ptr=None):
            if injected:
                xi = L.require_gpu_tensor(noise, "noise", promote=True)
                nd.xi, nd.ldxi = xi.data_ptr(), L.ld(xi)
            else:
                nd.seed = noise
            if form == "lagged":  # this launch leaves its partial rows, and finishes those of the previous launch (if any)
                k = launches[0]
                bd.energy_partials = part[k & 1]
                bd.energy_partials_prev = None if energy_ptr is None else part[(k - 1) & 1]
                bd.energy_prev, bd.energy_sums_prev = energy_ptr, slot_ptr
                launches[0] = k + 1
                energy_ptr = None
            elif form == "sums16":
                bd.energy_sums16 = slot_ptr
            elif form == "sums":
                bd.energy_sums = slot_ptr
            args[iu], args[iu + 1], args[io], args[io + 1], args[ie] = u_ptr, ldu, out_ptr, ldo, energy_ptr
            rc = fn(*args)
            if rc == 0 and form == "means":
                rc = means(energy_ptr, j, j, slot_ptr, stream)
            if rc:
                failed(rc)

        self.launch, self._failed = launch, failed

    def flush(self, u_ptr, ldu, energy_ptr, slot_ptr) -> None:
        """"lagged": finish the partial rows the LAST launch left into ``energy`` / ``slot`` (a small launch of its own, no
        step); ``u``: the particles that launch was given (shape and strides only)."""
        bd = L.BlockDesc()
        bd.block_cols, bd.eta = self.j, self.eta.data_ptr()
        bd.energy_partials_prev = self._part_ptr[(self._launches[0] - 1) & 1]
        bd.energy_prev, bd.energy_sums_prev, bd.energy_flush = energy_ptr, slot_ptr, 1
        nd = L.NoiseDesc()
        nd.kind = L.NOISE_NONE
        rc = self.route.call(bd, u_ptr, ldu, self.j, 0.0, nd, None, 0, L.OUT_DELTA, None, None, 0, self._stream)
        if rc:
            self._failed(rc)


class PLSBasis(ABC):
    """Function-space basis: initialise particles, energy potential, particle update, predictive samples."""

    def __init__(self, additional_predictive_noise_distribution: Optional[torch.distributions.Distribution] = None):
        self.additional_predictive_noise_distribution = additional_predictive_noise_distribution
        #: global column index of this rank's first particle (J-sharding, see distributed.py)
        self.j_offset = 0
        self._ws: dict = {}
        self.workspace_bytes = DEFAULT_WORKSPACE_BYTES

    @property
    def approximation_dimension(self) -> int:
        raise NotImplementedError

    # ---- noise -------------------------------------------------------------------------------------------------
    def _draw_noise_spec(self, noise: torch.Tensor | None) -> NoiseSpec:
        """The reference draws the step noise from torch's GLOBAL CPU generator (samplers.py:30-35 with
        generator=None), so callers make runs reproducible with set_seed() before the loop (runners.py:364).
        Same contract here: one 63-bit draw from that generator keys the on-device Philox stream of this step."""
        if noise is not None:
            return NoiseSpec(injected=noise)
        seed = int(torch.randint(0, 2**62, (1,), dtype=torch.int64).item())
        return NoiseSpec(seed=seed, step=0, j_offset=self.j_offset)

    def _workspace(self, nbytes: int, device) -> torch.Tensor:
        """The basis' own scratch buffer for EAGER calls: grown on demand, so its address may change between calls.
        Anything that freezes a pointer (a captured hipGraph) must own its buffer and pass it as ``workspace=``."""
        key = str(device)
        ws = self._ws.get(key)
        if ws is None or ws.numel() * 8 < nbytes:
            ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=device)
            self._ws[key] = ws
        return ws

    def _pick_workspace(self, workspace: torch.Tensor | None, nbytes: int, device) -> torch.Tensor:
        if workspace is None:
            return self._workspace(nbytes, device)
        L.require_gpu_tensor(workspace, "workspace")
        if workspace.numel() * 8 < nbytes:
            raise L.PlsHipError(f"workspace of {workspace.numel() * 8} bytes handed in, {nbytes} needed")
        return workspace

    # ---- the one-launch small-rank step (csrc/small_rank_step.h): what both bases keep for it ----------------------
    def _step_sync(self, j: int, device) -> torch.Tensor:
        """The zeroed arrival counters of the one-launch small-rank step (pls_block_desc.step_sync) for eager calls: one set per
        stream (launches on one stream are ordered; two streams must not share counters), grown on demand.  A launch leaves
        them zero; after a FAILED launch they are dropped (zero_step_sync) -- stale counts would make every later step wrong."""
        words = int(L.load().pls_step_sync_words(j))
        key = (str(device), L.stream_ptr())
        pool = self.__dict__.setdefault("_sync_pool", {})
        t = pool.get(key)
        if t is None or t.numel() < words:
            t = torch.zeros(max(words, 64), dtype=torch.int32, device=device)
            pool[key] = t
        return t

    def zero_step_sync(self) -> None:
        """Forget every counter set (after a failed or aborted launch): the next step allocates zeroed ones."""
        self.__dict__.pop("_sync_pool", None)

    def _eta_word(self, step_size: float, device) -> torch.Tensor:
        """``step_size`` as a device word (pls_block_desc.eta), remembered per value: an eager caller steps with the same size
        thousands of times, and a host -> device copy per call would cost more than the step."""
        words = self.__dict__.setdefault("_eta_words", {})
        key = (float(step_size), str(device))
        t = words.get(key)
        if t is None:
            if len(words) >= 64:
                words.clear()
            t = torch.full((1,), float(step_size), dtype=torch.float64, device=device)
            words[key] = t
        return t

    # ---- particles ---------------------------------------------------------------------------------------------
    def _initialise_particles_noise(self, number_of_particles: int, seed: int | None = None, mean: float = 0.0,
                                    stdev: float = 1.0) -> torch.Tensor:
        """basis/base.py:39-63: torch.normal on a CPU generator, size (M, J)."""
        generator = None
        if seed is not None:
            generator = torch.Generator().manual_seed(seed)
        return torch.normal(
            mean=mean, std=stdev, size=(self.approximation_dimension, number_of_particles), generator=generator
        )

    @abstractmethod
    def _initialise_particles(self, number_of_particles: int, noise_only: bool = True, seed: int | None = None) -> torch.Tensor:
        raise NotImplementedError

    def initialise_particles(self, number_of_particles: int, noise_only: bool = True, seed: int | None = None) -> torch.Tensor:
        """basis/base.py:81-102; the particles always live on the MI355X as float64."""
        return _dev(self._initialise_particles(number_of_particles=number_of_particles, noise_only=noise_only, seed=seed))

    @abstractmethod
    def calculate_untransformed_train_prediction_samples(self, particles: torch.Tensor) -> torch.Tensor:
        raise NotImplementedError

    @abstractmethod
    def calculate_energy_potential(self, particles: torch.Tensor, cost: torch.Tensor) -> float:
        raise NotImplementedError

    @abstractmethod
    def _calculate_particle_update(self, particles: torch.Tensor, cost_derivative: torch.Tensor, step_size: float,
                                   noise: torch.Tensor | None = None) -> torch.Tensor:
        raise NotImplementedError

    def calculate_particle_update(self, particles: torch.Tensor, cost_derivative: torch.Tensor, step_size: float,
                                  noise: torch.Tensor | None = None) -> torch.Tensor:
        """basis/base.py:143-163 (same assertion and message)."""
        assert (
            particles.shape[0] == self.approximation_dimension
        ), f"Particles have shape {particles.shape} but requires ({self.approximation_dimension}, J) dimension."
        extra = {} if noise is None else {"noise": noise}  # (subclasses with the reference's 3-argument signature keep working)
        return self._calculate_particle_update(
            particles=particles, cost_derivative=cost_derivative, step_size=step_size, **extra
        )

    @abstractmethod
    def sample_predictive_noise(self, particles: torch.Tensor, x: torch.Tensor):
        raise NotImplementedError

    @abstractmethod
    def predict_untransformed_samples(self, particles: torch.Tensor, x: torch.Tensor,
                                      noise: torch.Tensor | None = None) -> torch.Tensor:
        raise NotImplementedError

    # ---- fused native path (used by PLS when the cost is native) -------------------------------------------------
    def supports_fused_step(self) -> bool:
        return False

    #: ranks up to which a cost without the Gaussian algebra takes the small-rank kernels (csrc/small_rank.h, small_rank_step.h)
    SMALL_RANK_MAX = 128

    @staticmethod
    def _is_gaussian(cost, force_generic: bool = False, cd=None) -> bool:
        """The Gaussian cost with the identity link: the step has the closed Gaussian algebra (unless ``force_generic``);
        ``cd``: the cost's descriptor, if the caller holds it already."""
        cd = cost.desc() if cd is None else cd
        return cd.cost == L.COST_GAUSSIAN and cd.link == L.LINK_IDENTITY and not force_generic

    def _one_launch_rank(self, cost) -> bool:
        return (not self._is_gaussian(cost)) and 1 <= self.approximation_dimension <= self.SMALL_RANK_MAX

    def _route(self, cost, j: int, force_generic: bool = False, whitened: bool = False) -> StepRoute:
        """How one step of ``cost`` over ``j`` columns runs (StepRoute); ``whitened``: on whitened particles."""
        raise NotImplementedError

    def _general_ws_bytes(self, query, desc, j: int) -> int:
        """Workspace of a step entry's general route, whose size query (pls_*_step_workspace_bytes) is ``query``: the basis'
        budget (workspace_bytes), but at least what chunks of 128 rows need and at most what one chunk of all rows needs."""
        return max(query(desc, j, 128), min(query(desc, j, self._n), self.workspace_bytes))

    def step_workspace_bytes(self, cost, j: int, with_energy: bool, force_generic: bool = False) -> int:
        """Bytes fused_step asks of its workspace for ``j`` columns (graph captures allocate their own buffer)."""
        return self._route(cost, j, force_generic).workspace_bytes(with_energy)

    def _bind_step(self, cost, state: torch.Tensor, step_size: float, whitened: bool = False, energies: bool = True,
                   lagged: bool = True, injected: bool = False, new_state: bool = True) -> BoundStep:
        """The step of ``cost`` on particle buffers shaped like ``state`` as a BoundStep.  With ``energies`` it reports the
        energies of its input particles in the cheapest form the route has: the 16-column sums of the one-launch step, the
        lagged chunk sums of the Gaussian fast paths (``lagged``, else finished by the launch itself), or a mean launch."""
        r = self._route(cost, state.shape[1], whitened=whitened)
        if not energies:
            form = "none"
        elif r.one_launch:
            form = "sums16"
        elif r.lagged and lagged:
            form = "lagged"
        else:
            form = "sums" if r.sums else "means"
        return BoundStep(self, r, state, step_size, form, injected=injected, new_state=new_state)

    def fused_step(self, cost, particles: torch.Tensor, step_size: float, out: torch.Tensor | None = None,
                   new_state: bool = False, noise: NoiseSpec | None = None, force_generic: bool = False,
                   input_energy: torch.Tensor | None = None, blocks: BlockSpec | None = None,
                   workspace: torch.Tensor | None = None) -> torch.Tensor:
        """One whole Langevin step in libplship (the basis' step entry, see _route): returns dU, or U + dU when new_state.
        ``input_energy`` (J,) receives the per-particle energy of ``particles`` as a by-product.  ``blocks``: one step size
        per column block (the _blocks entry; ``step_size`` is then ignored).  ``workspace``: a caller-owned buffer -- a
        captured hipGraph freezes its address, so captures never use the basis' own growable scratch."""
        u = _rows_contiguous(L.require_gpu_tensor(particles, "particles", promote=True))
        return self._step(cost, u, step_size, out, new_state, noise, input_energy, blocks, workspace, force_generic)

    def _step(self, cost, u, step_size, out, new_state, noise, input_energy, blocks, workspace, force_generic=False,
              whitened=False) -> torch.Tensor:
        j = u.shape[1]
        if out is None:
            out = torch.empty_like(u, memory_format=torch.contiguous_format)
        else:  # (written as float64 through a raw pointer: a buffer of another dtype or shape must never get this far)
            L.require_gpu_tensor(out, "out")
            assert out.shape == u.shape, f"out has shape {tuple(out.shape)}, the particles {tuple(u.shape)}"
        if j == 0:
            return out
        assert out.data_ptr() != u.data_ptr(), "the step's out must not alias its particles"
        r = self._route(cost, j, force_generic, whitened)
        ws_bytes = r.workspace_bytes(input_energy is not None)
        ws = self._pick_workspace(workspace, ws_bytes, u.device) if ws_bytes else None
        nd = (noise if noise is not None else self._draw_noise_spec(None)).desc()
        bd = None if blocks is None else blocks.desc()
        if r.one_launch:
            # the one-launch small-rank step meets through zeroed counters: the basis' own (per stream) unless the caller's
            # BlockSpec brings some -- without them the library puts a memset node in front of every launch
            if bd is None:
                bd = L.BlockDesc()
                bd.block_cols, bd.eta = j, self._eta_word(step_size, u.device).data_ptr()
            if not bd.step_sync:
                bd.step_sync = self._step_sync(j, u.device).data_ptr()
        try:
            L.check(r.call(bd, u.data_ptr(), L.ld(u), j, float(step_size), nd, out.data_ptr(), L.ld(out),
                           L.OUT_NEW_STATE if new_state else L.OUT_DELTA, L.ptr(input_energy), L.ptr(ws), ws_bytes,
                           L.stream_ptr()),
                    r.entry if bd is None else r.blocks_entry)
        except L.PlsHipError:
            self.zero_step_sync()
            raise
        return out


def _rows_contiguous(t: torch.Tensor) -> torch.Tensor:
    assert t.dim() == 2, "expected a 2-D tensor"
    return t if t.stride(1) == 1 or t.shape[1] <= 1 and t.is_contiguous() else t.contiguous()


def padded_ld(cols: int) -> int:
    """Leading dimension rounded up to 16 doubles (128 B): every row of a library-owned matrix starts on a full line."""
    return (cols + 15) // 16 * 16


def alloc_matrix(rows: int, cols: int, device) -> torch.Tensor:
    """(rows, cols) float64 view with a padded leading dimension."""
    ldm = padded_ld(cols)
    return torch.empty((rows, ldm), dtype=torch.float64, device=device)[:, :cols]

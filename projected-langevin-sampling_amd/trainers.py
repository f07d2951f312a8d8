"""Caller of the hot path (drop-in for experiments/trainers.py:139-162 and experiments/early_stopper.py:4-24)."""
from __future__ import annotations

import time
from typing import List, Tuple

import numpy as np
import torch

from . import _lib as L
from . import _ops
from .projected_langevin_sampling import PLS


class EarlyStopper:
    """Stops when the simulated time without an improving loss reaches ``patience`` (early_stopper.py:4-24)."""

    def __init__(self, patience: float = 1e-4):
        self.patience = patience
        self.simulation_time = 0
        self.min_loss = float("inf")

    def should_stop(self, loss: float, step_size: float) -> bool:
        if not np.isfinite(loss):
            return True
        elif loss >= self.min_loss:
            self.simulation_time += step_size
            return self.simulation_time >= self.patience
        else:
            self.min_loss = loss
            self.simulation_time = 0
            return False


def mean_from_chunk_sums(sums, count: int) -> float:
    """Mean energy from the 256-column chunk sums the step's finishing launch leaves (pls_block_desc.energy_sums: what
    pls_block_means computes, bit for bit) or from the 16-column sums of the one-launch small-rank step
    (pls_block_desc.energy_sums16): the entries added in ascending order, divided by the particle count."""
    if isinstance(sums, np.ndarray) and sums.shape[0] > 16:
        # (a cumulative sum is strictly sequential: the loop below, vectorised; the loop starts at 0.0 and np.cumsum at
        # sums[0], which differ when every sum is -0.0: the + 0.0 is the kernel's +0.0 there and changes nothing else)
        return (float(np.cumsum(sums)[-1]) + 0.0) / count
    total = 0.0
    for v in sums:
        total += float(v)
    return total / count


class _LoopSpace:
    """The coordinates a training loop keeps its particles in between steps.  Identity for every basis but one: the
    inducing-point basis under the Gaussian cost with the identity link, whose step is ONE contraction per iteration in
    whitened coordinates S = Lc^-1 U (InducingPointBasis.whitened_step: 2 M^2 J flop) against forward solve + contraction
    + Lc dS per call (4 M^2 J) -- the loop whitens once, steps S, and maps back once (same chain, same noise counters,
    same energies to rounding: tests/test_gpu_whitened.py).  Injected noise matrices are coloured (N(0, k(Z,Z)) samples
    the reference's sampler would have drawn), so a loop that injects them stays in the original coordinates."""

    def __init__(self, pls: PLS, noises, j: int = 0):
        basis, cost = pls.basis, pls.cost
        self.pls = pls
        can = bool(noises is None and getattr(basis, "whitened", False) and hasattr(basis, "whitened_step")
                   and getattr(cost, "is_native", lambda: False)())
        self.whitened = bool(can and basis._is_gaussian(cost, False))
        # ... and, round 5, the same basis under ANY native cost on at most 128 inducing points while the problem is launch-bound:
        # in whitened coordinates the prior is M more rows of the forward operand and the noise is white, so an iteration is
        # ONE launch (InducingPointBasis.whitened_generic_applies) instead of solve + coloured noise + step -- same draws
        self.whitened_generic = bool(can and not self.whitened and j > 0
                                     and getattr(basis, "whitened_generic_applies", lambda c, n: False)(cost, j))
        self.whitened = self.whitened or self.whitened_generic

    def enter(self, particles: torch.Tensor) -> torch.Tensor:
        return self.pls.basis.whiten(particles) if self.whitened else particles

    def step(self, state, step_size, out, noise, input_energy):
        basis, cost = self.pls.basis, self.pls.cost
        fn = basis.whitened_step if self.whitened else basis.fused_step
        return fn(cost, state, float(step_size), out=out, new_state=True, noise=noise, input_energy=input_energy)

    def bind(self, state, step_size, injected: bool):
        """the loop's step call with its energies, bound once (basis._bind_step: a BoundStep)"""
        return self.pls.basis._bind_step(self.pls.cost, state, step_size, whitened=self.whitened, lagged=LAGGED_ENERGIES,
                                         injected=injected)

    def energy(self, state) -> torch.Tensor:
        if self.whitened:
            return self.pls.basis.whitened_particle_energy(self.pls.cost, state)
        return self.pls.particle_energy_potential(state)

    def leave(self, state: torch.Tensor, particles: torch.Tensor) -> None:
        """final state -> the caller's particle tensor"""
        if self.whitened:
            self.pls.basis.unwhiten(state, out=particles)
        elif state.data_ptr() != particles.data_ptr():
            particles.copy_(state)


def _mean_energy(e: torch.Tensor) -> float:
    """Mean over the particles of the per-particle energies (orthonormal.py:126's .mean().item()): libplship's fixed-order
    reduction for device vectors, so that every loop variant (plain, pipelined, captured) reports identical values."""
    return _ops.block_means(e).item() if e.is_cuda else e.mean().item()


def train_pls(
    pls: PLS,
    particles: torch.Tensor,
    number_of_epochs: int,
    step_size: float,
    early_stopper_patience: float,
    tqdm_desc: str | None = None,
    noises: List[torch.Tensor] | None = None,
    energy_reduce=None,
) -> Tuple[torch.Tensor, List[float]]:
    """trainers.py:139-162: update, in-place add, energy, early stop.

    ``noises`` (extension) injects the noise of each step; ``energy_reduce`` (extension) maps the local
    per-particle energy vector to the global mean (distributed.mean_over_particles for J-sharded runs).

    When the step kernel can emit the energy of its input particles as a by-product (Gaussian/identity on the
    orthonormal basis), the loop is software-pipelined: the launch of step t+1 also produces the energy the reference
    evaluates after step t, so every iteration is ONE kernel.  Results (particles, energy list, stop index, torch RNG
    state) are those of the plain loop: a step launched speculatively past the stop is discarded."""
    if particles.is_cuda and particles.dtype in L.PROMOTED_DTYPES:
        # float32 particles: the run is carried in float64 (one rounding at the end instead of one per step) and the caller's
        # tensor receives the final state, which is also what is returned -- trainers.py:157 mutates its argument
        state, energy_potentials = train_pls(pls, particles.double(), number_of_epochs, step_size, early_stopper_patience,
                                             tqdm_desc, noises, energy_reduce)
        particles.copy_(state)
        return particles, energy_potentials
    reduce = energy_reduce if energy_reduce is not None else _mean_energy
    early_stopper = EarlyStopper(patience=early_stopper_patience)
    energy_potentials: List[float] = []
    pipelined = (
        number_of_epochs > 0 and pls._fused() and getattr(pls.basis, "supports_input_energy", lambda c: False)(pls.cost)
    )
    if not pipelined:
        for t in range(number_of_epochs):
            pls.step_(particles, step_size, noise=None if noises is None else noises[t])
            energy_potential = reduce(pls.particle_energy_potential(particles))
            if early_stopper.should_stop(loss=energy_potential, step_size=step_size):
                break
            energy_potentials.append(energy_potential)
        return particles, energy_potentials

    from .basis.base import NoiseSpec

    if particles.is_cuda and (energy_reduce is None or hasattr(energy_reduce, "reduce_local_sum")):
        # (a J-sharded run hands in distributed.EnergyMean: the ranks' local sums meet on the host, the GPU queues stay full)
        return _train_pls_in_flight(pls, particles, number_of_epochs, step_size, early_stopper, noises, mean=energy_reduce)

    space = _LoopSpace(pls, noises, particles.shape[1])
    cur = space.enter(particles)
    nxt = torch.empty_like(particles, memory_format=torch.contiguous_format)
    e_in = torch.empty(particles.shape[1], dtype=torch.float64, device=particles.device)
    stopped = False
    for t in range(number_of_epochs):
        rng_state = torch.get_rng_state()  # the speculative launch below may have to be un-drawn
        spec = NoiseSpec(injected=noises[t]) if noises is not None else None
        space.step(cur, step_size, nxt, spec, e_in)
        if t >= 1:  # e_in = energy of `cur`, i.e. of the particles after update t-1 (trainers.py:158)
            energy_potential = reduce(e_in)
            if early_stopper.should_stop(loss=energy_potential, step_size=step_size):
                torch.set_rng_state(rng_state)
                stopped = True
                break
            energy_potentials.append(energy_potential)
        cur, nxt = nxt, cur
    if not stopped:  # energy after the last update
        energy_potential = reduce(space.energy(cur))
        if not early_stopper.should_stop(loss=energy_potential, step_size=step_size):
            energy_potentials.append(energy_potential)
    space.leave(cur, particles)
    return particles, energy_potentials


#: step launches the pipelined loop keeps queued ahead of the energy it is waiting for (>= 2).  Two keep the GPU busy over
#: the host's ordinary round trip (~30 us); on a shared host the Python thread is now and then descheduled for milliseconds
#: (measured on the GPU boxes: the same loop 0.275 or 0.31 ms per iteration from one repetition to the next, the host's
#: share of an iteration 29 or 63 us, tools/train_loop_probe.py), and a queue of eight 0.27 ms launches rides that out.
#: Costs depth + 1 particle buffers and up to `depth` speculative launches past the stop (discarded).
IN_FLIGHT_DEPTH = 8
#: Gaussian fast paths: launch k + 1 finishes the energies of launch k at its start (pls_block_desc.energy_partials ...), so
#: that no launch carries the reduction's serial tail; False: every launch finishes its own (energy_sync)
LAGGED_ENERGIES = True
#: ... as long as the rotating particle buffers stay below this many bytes (depth is reduced, never below 2)
IN_FLIGHT_BUFFER_BYTES = 4 << 30


def _train_pls_in_flight(pls: PLS, particles: torch.Tensor, number_of_epochs: int, step_size: float,
                         early_stopper: EarlyStopper, noises, depth: int | None = None, mean=None) -> Tuple[torch.Tensor, List[float]]:
    """The pipelined loop with `depth` step launches queued: launch k computes U_{k+1} from U_k and, as a by-product, the
    energy of U_k (or, lagged, finishes that of U_{k-1}), which travels to a slot of pinned host memory: the sums of its
    column chunks, or its mean (basis._bind_step decides the form).  The host polls that slot while launches k+1 .. k+depth-1
    are already queued behind it -- so the GPU never idles over the host's round trip (early-stop logic + next launch, ~30 us
    against a 270 us step at configs[1]) nor over a descheduled host thread.  At the reference's own problem sizes the host's
    share of an iteration bounds the loop (a 10 us kernel against 20 us of Python): the step call is bound once, the buffers'
    addresses are looked up once, the slots are polled through numpy views, and the per-step keys are drawn from torch's
    global generator in batches -- the same stream of draws as one per step.  depth + 1 particle buffers rotate, so the
    launches made speculatively past the stop never touch the returned state, and the generator is left where the plain
    loop leaves it: one draw per executed step.  Same particles, energies and stop index as the plain loop
    (tests/test_gpu_parity.py)."""
    from .basis.base import UNWRITTEN_ENERGY_BITS as UNWRITTEN

    T = number_of_epochs
    j = particles.shape[1]
    if depth is None:
        depth = IN_FLIGHT_DEPTH
        while depth > 2 and (depth + 1) * particles.numel() * 8 > IN_FLIGHT_BUFFER_BYTES:
            depth -= 1
    depth = max(2, min(int(depth), max(T, 2)))
    NB = depth + 1  # rotating slots: particle buffers, energy vectors, host slots
    space = _LoopSpace(pls, noises, j)
    first = space.enter(particles)
    if first.stride(1) != 1:  # (the launches take row-contiguous buffers; leave() copies the final state back)
        first = first.contiguous()
    bufs = [first] + [torch.empty_like(particles, memory_format=torch.contiguous_format) for _ in range(NB - 1)]
    e_dev = [torch.empty(j, dtype=torch.float64, device=particles.device) for _ in range(NB)]
    step = space.bind(first, step_size, injected=noises is not None)
    launch_step = step.launch
    lag = 1 if step.reports_previous else 0  # launch k reports the energies of U_{k - lag}
    means = step.form == "means"  # (a slot holds the mean; otherwise the sums of column chunks)
    nchunk = step.slot_doubles
    host = torch.empty(NB * nchunk, dtype=torch.float64).pin_memory()
    host_ptr = host.data_ptr()  # (hipHostMalloc'ed by torch: host and device addresses coincide)
    # No event per launch.  An event record puts a barrier packet between the finishing launch and the next step (5.8 us of
    # idle GPU per iteration in rocprofv3's trace, 2 % of a 0.27 ms iteration); instead the host fills a slot with a NaN of a
    # payload no computation produces before it queues the launch, and reads the slot once every entry has been overwritten
    # (each entry is ONE 8-byte store into coherent pinned memory; a diverged run's NaN / inf energies are ordinary values here)
    host_np = host.numpy()  # (shares the pinned pages)
    host_bits = host_np.view(np.int64)
    buf_ptr, buf_ld = [b.data_ptr() for b in bufs], [L.ld(b) for b in bufs]
    e_ptr = [e.data_ptr() for e in e_dev]
    keys: List[int] = []
    rng_start = torch.get_rng_state() if noises is None else None
    launched = 0
    flushed = False

    def launch():
        nonlocal launched
        k = launched
        if noises is None:
            if k >= len(keys):
                keys.extend(torch.randint(0, 2**62, (256,), dtype=torch.int64).tolist())
            noise = keys[k]
        else:
            noise = noises[k]
        a, b, s = k % NB, (k + 1) % NB, (k - lag) % NB
        if k >= lag:
            host_bits[s * nchunk:(s + 1) * nchunk] = UNWRITTEN
            launch_step(buf_ptr[a], buf_ld[a], buf_ptr[b], buf_ld[b], noise, e_ptr[s], host_ptr + 8 * nchunk * s)
        else:
            launch_step(buf_ptr[a], buf_ld[a], buf_ptr[b], buf_ld[b], noise)
        launched += 1

    def read_energy(slot: int) -> float:
        vals = host_np[slot * nchunk:(slot + 1) * nchunk]
        if mean is not None:  # J-sharded run (distributed.EnergyMean): the local SUM goes to the ranks' host-side exchange
            return mean.reduce_local_sum(float(vals[0]) * j if means else mean_from_chunk_sums(vals, 1))
        return float(vals[0]) if means else mean_from_chunk_sums(vals, j)

    def wait_for(slot: int) -> None:
        bits = host_bits[slot * nchunk:(slot + 1) * nchunk]
        spins = 0
        while bool((bits == UNWRITTEN).any()):
            spins += 1
            if spins > 1024:  # far beyond a fast-path step (tens to hundreds of microseconds): stop burning the core
                time.sleep(1e-4)
            if spins % 4096 == 0 and torch.cuda.current_stream().query():  # the queue has drained and the slot is still
                if bool((bits == UNWRITTEN).any()):                       # unwritten: a failed launch, not a slow one
                    raise RuntimeError("train_pls: the step launch did not deliver its energy sums")

    energy_potentials: List[float] = []
    final = None
    keys_used = T  # (the plain loop draws one key per step it executes: T, or t + 1 when iteration t stops it)
    try:
        for t in range(T):  # iteration t of the plain loop: update t done (U_{t+1}), its energy E(U_{t+1}) wanted
            # launch t+1 carries E(U_{t+1}); t+2 .. t+depth keep the queue non-empty.  Launch k writes slot (k+1) % NB and
            # the stop below may return slot (t+1) % NB: k + 1 - (t + 1) <= depth < NB, so that slot is never overwritten
            while launched < T and launched <= t + depth:
                launch()
            if lag and launched == T and not flushed:
                # every step is queued: E(U_{T-1}) has no following launch to ride on -- a small finishing launch of its own
                s = (T - 1) % NB
                host_bits[s * nchunk:(s + 1) * nchunk] = UNWRITTEN
                step.flush(buf_ptr[s], buf_ld[s], e_ptr[s], host_ptr + 8 * nchunk * s)
                flushed = True
            if t + 1 < T:
                wait_for((t + 1) % NB)
                energy_potential = read_energy((t + 1) % NB)
            else:  # the energy after the last update has no following launch to ride on
                last = space.energy(bufs[T % NB])
                energy_potential = _mean_energy(last) if mean is None else mean.reduce_local_sum(last.sum().item())
            if early_stopper.should_stop(loss=energy_potential, step_size=step_size):
                keys_used = t + 1
                final = bufs[(t + 1) % NB]
                break
            energy_potentials.append(energy_potential)
    except BaseException as exc:
        # a J-sharded run: the other ranks are polling for this rank's next energy sum -- tell them it will not come
        if mean is not None and hasattr(mean, "abort"):
            mean.abort(repr(exc)[:200])
        raise
    finally:
        # up to `depth` launches are still queued: they write the pinned slots and the rotating buffers, which must not go
        # back to torch's allocators (on ANY exit: a raising early stopper, a failed launch) before they have drained
        torch.cuda.current_stream().synchronize()
    if rng_start is not None:  # leave torch's generator where one draw per executed step leaves it
        torch.set_rng_state(rng_start)
        if keys_used > 0:
            torch.randint(0, 2**62, (keys_used,), dtype=torch.int64)
    if final is None:
        final = bufs[T % NB]
    space.leave(final, particles)
    return particles, energy_potentials


def train_pls_captured(pls: PLS, particles: torch.Tensor, number_of_epochs: int, step_size: float,
                       early_stopper_patience: float, steps_per_replay: int = 16, seed: int | None = None
                       ) -> Tuple[torch.Tensor, List[float]]:
    """train_pls for launch-bound problems (extension): K steps and their energies per hipGraph replay
    (graph.CapturedTraining).  Same loop semantics as experiments/trainers.py:139-162 -- update, energy of the updated
    particles, early stop, the failing update is kept -- over the library's counter-based noise stream: ``seed`` (one
    draw from torch's global generator if None) keys it, step t uses counter t.  The result equals the eager loop over
    that stream exactly (an overshooting replay is rolled back and re-run up to the stop index)."""
    from .graph import CapturedTraining

    if seed is None:
        seed = int(torch.randint(0, 2**63 - 1, (1,)).item())
    early_stopper = EarlyStopper(patience=early_stopper_patience)
    energies: List[float] = []
    T, K = number_of_epochs, max(1, min(steps_per_replay, number_of_epochs))
    if T == 0:
        return particles, energies
    cap = CapturedTraining(pls, particles, step_size, K, seed)
    t = 0  # next plain-loop iteration to judge: needs E(U_{t+1})
    while t < T:
        k0 = cap.steps_done
        if k0 + K <= T:  # a full replay: launches k0 .. k0+K-1 report E(U_k0) .. E(U_{k0+K-1})
            known = cap.replay().tolist()
        else:  # fewer than K steps left: finish eagerly, one energy per step
            known = None
        if known is not None:
            stop_at = None
            for s, e in enumerate(known):
                it = k0 + s - 1  # E(U_{k0+s}) closes plain-loop iteration k0+s-1
                if it < 0:
                    continue  # E(U_0): the plain loop never looks at it
                if early_stopper.should_stop(loss=e, step_size=step_size):
                    stop_at = it
                    break
                energies.append(e)
                t = it + 1
            if stop_at is not None:  # keep U_{stop_at+1}: rewind the replay, roll forward eagerly
                cap.roll_back()
                cap.eager_steps(stop_at + 1 - cap.steps_done)
                return particles, energies
        else:
            while t < T:
                if cap.steps_done < t + 1:
                    cap.eager_steps(t + 1 - cap.steps_done)
                e = _mean_energy(pls.particle_energy_potential(particles))
                if early_stopper.should_stop(loss=e, step_size=step_size):
                    return particles, energies
                energies.append(e)
                t += 1
            return particles, energies
        if cap.steps_done == T:  # all updates done; E(U_T) has no following launch to ride on
            e = _mean_energy(pls.particle_energy_potential(particles))
            if not early_stopper.should_stop(loss=e, step_size=step_size):
                energies.append(e)
            return particles, energies
    return particles, energies


def epoch_batches(n: int, batch_size: int) -> List[torch.Tensor]:
    """The index batches of one epoch of the reference's SVGP loader (experiments/trainers.py:112-113): a real
    ``DataLoader(TensorDataset(arange(n)), batch_size, shuffle=True)`` is iterated, so torch's global generator is consumed
    exactly as the reference's loader over (x, y) consumes it, and batch k lists the rows that loader would yield as its
    batch k (the last one ragged)."""
    from torch.utils.data import DataLoader, TensorDataset

    loader = DataLoader(TensorDataset(torch.arange(n)), batch_size=batch_size, shuffle=True)
    return [batch[0] for batch in loader]


def train_svgp(x: torch.Tensor, y: torch.Tensor, x_induce: torch.Tensor, kernel, seed: int, number_of_epochs: int,
               batch_size: int, learning_rate: float, early_stopper_patience: float, likelihood_noise: float | None = None,
               learn_inducing_locations: bool = False, learn_kernel_parameters: bool = False, train_noise: bool = True,
               mean_init_std: float = 1e-3, likelihood=None):
    """experiments/trainers.py:55-136 with ``is_fixed=True`` (what every driver of the reference runs): seed, the model, and per
    epoch every minibatch SGD step on loss = -ELBO followed by the full-data loss -- ONE library call (pls_svgp_sgd_epoch)
    and one host read --, the early-stopper check before the loss is recorded.  Returns (model, losses); (None, None) when
    a loss is not finite or k(Z, Z) stays non-PSD (the reference's ``except ValueError``).  ``train_noise=False`` freezes
    the likelihood noise (train_svgp_for_profiler, experiments/profiler/main.py:106-107).  ``likelihood``: None (Gaussian) or
    a likelihood object, as the drivers pass ``BernoulliLikelihood()`` and a ``StudentTLikelihood``; ``likelihood_noise``
    with a Bernoulli likelihood raises AttributeError (the reference sets ``likelihood.noise``), with a Student-t one it is
    the starting scale^2."""
    from ._chol import NotPSDError
    from .gaussian_process import SVGP
    from .utils import set_seed

    if learn_kernel_parameters:
        raise NotImplementedError("train_svgp: learn_kernel_parameters=True is not supported: the kernel and the inducing "
                                  "points are fixed (the reference's is_fixed=True)")
    set_seed(seed)
    model = SVGP(kernel, x_induce, likelihood="gaussian" if likelihood is None else likelihood, noise=likelihood_noise,
                 learn_inducing_locations=learn_inducing_locations, mean_init_std=mean_init_std)
    try:
        model.fit_data(x, y)
    except NotPSDError as e:
        print(e)
        return None, None
    early_stopper = EarlyStopper(patience=early_stopper_patience)
    losses: List[float] = []
    for _ in range(number_of_epochs):
        perm = torch.cat(epoch_batches(model.n, batch_size))
        loss = model.sgd_epoch(perm, batch_size, learning_rate, train_mean=True, train_noise=train_noise).item()
        if not np.isfinite(loss):
            print(f"train_svgp: the loss is {loss}")
            return None, None
        if early_stopper.should_stop(loss=loss, step_size=learning_rate):
            break
        losses.append(loss)
    return model, losses

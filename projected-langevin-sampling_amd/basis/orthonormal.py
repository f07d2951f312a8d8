"""Orthonormal basis (drop-in for src/projected_langevin_sampling/basis/orthonormal.py:10-244)."""
from __future__ import annotations

import torch

from .. import _lib as L
from .. import _ops
from ..kernel import PLSKernel, _dev
from ..samplers import sample_multivariate_normal
from .base import BlockSpec, NoiseSpec, PLSBasis, StepRoute, _rows_contiguous, alloc_matrix


class OrthonormalBasis(PLSBasis):
    """Particles live in the eigenbasis of k(Z,Z)/M (orthonormal.py:22-68).

    Setup (once): k(Z,Z), k(Z,X) on the GPU; torch.linalg.eigh like the reference, on the device the Gram matrix lives on
    (``eigh_device="cpu"`` / ``samplers.DEFAULT_EIGH_DEVICE`` select host LAPACK, the reference's CPU path; the
    eigenvector gauge is implementation defined, so parity runs may pass ``spectrum=(eigenvalues, eigenvectors)``;
    ``eigh_device="plship"`` runs libplship's own solver, pls_sym_eigh: one gauge, the same bits on every rank); then the projection
    A = V~^T k(Z,X) and its transpose are built once on the GPU instead of re-associating three matrices per step
    (orthonormal.py:106-108, :151-155)."""

    def __init__(
        self,
        kernel: PLSKernel,
        x_induce: torch.Tensor,
        x_train: torch.Tensor,
        eigenvalue_threshold: float = 0.0,
        additional_predictive_noise_distribution: torch.distributions.Distribution | None = None,
        spectrum: tuple[torch.Tensor, torch.Tensor] | None = None,
        keep_gram: bool = True,
        verbose: bool = True,
        eigh_device: str | None = None,
        setup_times: dict | None = None,
        group=None,
        canonical_signs: bool | None = None,
    ):
        super().__init__(additional_predictive_noise_distribution=additional_predictive_noise_distribution)
        import time

        #: seconds per setup phase (gram / eigh / projection), filled when ``setup_times`` is a dict (each phase is then
        #: closed by a device synchronisation; bench.py reports them as config.setup_breakdown)
        self.setup_times = setup_times

        def lap(name, t0):
            if setup_times is not None:
                torch.cuda.synchronize()
                setup_times[name] = setup_times.get(name, 0.0) + time.perf_counter() - t0
            return time.perf_counter()

        t_lap = time.perf_counter()
        self.kernel = kernel
        self.x_induce = x_induce  # (M, D)
        m = x_induce.shape[0]
        # (inputs go to the device ONCE: each host -> device copy costs ~14 us, and at the sizes of the reference's own
        # benchmark -- experiments/profiler/config.yaml: 10 inducing points, 100 data points -- copies ARE the construction)
        z_dev, x_dev = _dev(x_induce), _dev(x_train)
        self.base_gram_induce = self.kernel.base_kernel(x1=z_dev, x2=z_dev)  # k(Z,Z) (M, M)   :36-38
        base_gram_induce_train = self.kernel.base_kernel(x1=z_dev, x2=x_dev)  # k(Z,X) (M, N)   :39-41
        dev = self.base_gram_induce.device
        t_lap = lap("gram_s", t_lap)
        if spectrum is None:
            # :46-48, torch.linalg.eigh where the matrix lives unless told otherwise (samplers.DEFAULT_EIGH_DEVICE).  "cpu"
            # is the reference's CPU path (host LAPACK: 0.9 s at M = 1024, 21 s at 4096 on a GPU box's host share; the
            # whole setup otherwise takes 0.1 s); on the GPU the same factorisation takes 0.03 / 0.15 s -- another,
            # equally valid, eigenvector gauge (signs made canonical, basis/spectrum.py), and eigenvalues that differ in
            # the last bits.  A J-sharded run passes ``group`` (True = the default process group, or a ProcessGroup): ONE
            # process decides -- rank 0 of the group factorises and broadcasts (lambda, V) after the group has checked
            # that all ranks hold the same k(Z,Z)/M -- so every rank keeps the same count and the same gauge, bit for
            # bit.  ``group=None`` (default) enters no collective: the reference's local eigh (basis/spectrum.py).
            from ..samplers import resolve_eigh_device
            from .spectrum import shared_spectrum

            g = (1 / m) * self.base_gram_induce
            eigenvalues, eigenvectors = shared_spectrum(g, resolve_eigh_device(eigh_device, g), group=group,
                                                        canonical_signs=canonical_signs)
        else:
            eigenvalues, eigenvectors = (t.detach().cpu().to(torch.float64) for t in spectrum)
        t_lap = lap("eigh_s", t_lap)
        idx = torch.where(eigenvalues > eigenvalue_threshold)[0]  # :52
        eigenvalues = eigenvalues[idx].real
        eigenvectors = eigenvectors[:, idx].real
        if verbose:
            print(f"Number of eigenvalues kept: {eigenvalues.shape[0]} out of {m}")  # :58-60
        mk = eigenvalues.shape[0]
        from .spectrum import assert_same_count

        assert_same_count(mk, group)  # (also with spectrum=: gather_particles / predictive_moments need one M_k)
        scaled = torch.multiply(torch.reciprocal(torch.sqrt(mk * eigenvalues))[None, :], eigenvectors)  # :63-68
        # one upload for the four host results (eigenvalues, eigenvectors, V~, V~ diag(lambda)), carved into views that each
        # start on a 128-byte line
        parts = [eigenvalues.reshape(-1), eigenvectors.reshape(-1), scaled.reshape(-1), (scaled * eigenvalues[None, :]).reshape(-1)]
        offs, total = [], 0
        for t in parts:
            offs.append(total)
            total += (t.numel() + 15) // 16 * 16
        flat = torch.zeros(max(total, 1), dtype=torch.float64)
        for t, o in zip(parts, offs):
            flat[o:o + t.numel()] = t
        flat = _dev(flat)
        self.eigenvalues = flat[offs[0]:offs[0] + mk]
        self.eigenvectors = flat[offs[1]:offs[1] + m * mk].view(m, mk)
        self.scaled_eigenvectors = flat[offs[2]:offs[2] + m * mk].view(m, mk)  # (M, Mk)
        self._scaled_eigenvectors_lam = flat[offs[3]:offs[3] + m * mk].view(m, mk)  # V~ diag(lambda), prediction only
        n = base_gram_induce_train.shape[1]
        self._n = n
        self._A = alloc_matrix(mk, n, dev)
        self._At = alloc_matrix(n, mk, dev)
        if mk > 0:
            L.check(
                L.load().pls_onb_build_projection(
                    self.scaled_eigenvectors.data_ptr(), L.ld(self.scaled_eigenvectors), base_gram_induce_train.data_ptr(),
                    L.ld(base_gram_induce_train), m, mk, n, self._A.data_ptr(), L.ld(self._A), self._At.data_ptr(),
                    L.ld(self._At), L.stream_ptr(),
                ),
                "pls_onb_build_projection",
            )
        self.base_gram_induce_train = base_gram_induce_train if keep_gram else None
        lap("projection_s", t_lap)
        self._B = None  # Gaussian fast path constants, keyed by the y they were built from
        self._c = None
        self._gauss_key = None

    @classmethod
    def from_projection(cls, projection: torch.Tensor, eigenvalues: torch.Tensor,
                        poison_padding: bool = False) -> "OrthonormalBasis":
        """A basis given directly by its projection A = V~^T k(Z,X) (M_k, N) and eigenvalues (M_k,): everything on the
        per-step path works (forward, update, fused step, energy); prediction needs the kernel and is unavailable.
        ``poison_padding`` fills the alignment padding of the device copies with NaN (tests: padding must never be
        read as data)."""
        a = L.require_gpu_tensor(projection, "projection")
        lam = L.require_gpu_tensor(eigenvalues, "eigenvalues").contiguous()
        mk, n = a.shape
        assert lam.shape == (mk,), "one eigenvalue per row of the projection"
        self = cls.__new__(cls)
        PLSBasis.__init__(self, additional_predictive_noise_distribution=None)
        self.kernel = None
        self.x_induce = None
        self.base_gram_induce = None
        self.base_gram_induce_train = None
        self.eigenvalues = lam
        self.eigenvectors = None
        self.scaled_eigenvectors = None
        self._scaled_eigenvectors_lam = None
        self._n = n
        self._A = alloc_matrix(mk, n, a.device)
        self._At = alloc_matrix(n, mk, a.device)
        if poison_padding:
            self._A._base.fill_(float("nan"))
            self._At._base.fill_(float("nan"))
        self._A.copy_(a)
        self._At.copy_(a.T)
        self._B = None
        self._c = None
        self._gauss_key = None
        return self

    @property
    def approximation_dimension(self) -> int:
        return self.eigenvalues.shape[0]  # :70-76

    def spectrum_fingerprint(self) -> dict | None:
        """What a checkpoint records about the eigenvector gauge its particles are coordinates in (basis/spectrum.py);
        None for a basis without eigenvectors (from_projection)."""
        if self.eigenvectors is None:
            return None
        fp = self.__dict__.get("_fingerprint")
        if fp is None:
            from .spectrum import spectrum_fingerprint

            fp = self._fingerprint = spectrum_fingerprint(self.eigenvalues, self.eigenvectors)
        return fp

    # ---- descriptors ---------------------------------------------------------------------------------------------
    def _desc(self, with_gaussian: bool = False) -> L.OnbDesc:
        key = (bool(with_gaussian and self._B is not None), self._A.data_ptr(), None if self._B is None else self._B.data_ptr())
        cached = self.__dict__.get("_desc_cache")
        if cached is not None and cached[0] == key:
            return cached[1]
        d = self._build_desc(with_gaussian)
        self._desc_cache = (key, d)
        return d

    def _build_desc(self, with_gaussian: bool) -> L.OnbDesc:
        d = L.OnbDesc()
        d.mk, d.n = self.approximation_dimension, self._n
        d.A, d.lda = self._A.data_ptr(), L.ld(self._A)
        d.At, d.ldat = self._At.data_ptr(), L.ld(self._At)
        d.lam = self.eigenvalues.data_ptr()
        if with_gaussian and self._B is not None:
            d.B, d.ldb, d.c = self._B.data_ptr(), L.ld(self._B), self._c.data_ptr()
        return d

    def prepare_gaussian(self, y_dev: torch.Tensor) -> None:
        """B = A A^T, c = A y: turns the Gaussian/identity step into the M_k x M_k x J contraction (README.md:9)."""
        key = (y_dev.data_ptr(), y_dev._version)
        if self._gauss_key == key:
            return
        mk = self.approximation_dimension
        self._B = alloc_matrix(mk, mk, y_dev.device)
        self._c = torch.empty(mk + 1, dtype=torch.float64, device=y_dev.device)  # A y, then y^T y
        L.check(
            L.load().pls_onb_build_gaussian(self._desc(), y_dev.data_ptr(), self._B.data_ptr(), L.ld(self._B),
                                            self._c.data_ptr(), L.stream_ptr()),
            "pls_onb_build_gaussian",
        )
        self._gauss_key = key

    # ---- reference API ---------------------------------------------------------------------------------------------
    def _initialise_particles(self, number_of_particles: int, noise_only: bool = True, seed: int | None = None) -> torch.Tensor:
        if not noise_only:
            raise ValueError("For ONB base, noise_only must be True.")  # :91-92
        return self._initialise_particles_noise(number_of_particles=number_of_particles, seed=seed)

    def calculate_untransformed_train_prediction_samples(self, particles: torch.Tensor) -> torch.Tensor:
        """F = k(X,Z) V~ U = A^T U  (N, J)  (:98-108)."""
        u = _rows_contiguous(L.require_gpu_tensor(particles, "particles", promote=True))
        j = u.shape[1]
        f = torch.empty((self._n, j), dtype=torch.float64, device=u.device)
        L.check(
            L.load().pls_onb_forward(self._desc(), u.data_ptr(), L.ld(u), j, f.data_ptr(), max(j, 1), L.stream_ptr()),
            "pls_onb_forward",
        )
        return f

    def particle_energy_potential(self, particles: torch.Tensor, cost: torch.Tensor | None) -> torch.Tensor:
        """Per-particle energy e_j = cost_j + 1/2 sum_m U_mj^2 / lambda_m  (J,)  (:120-125)."""
        u = _rows_contiguous(L.require_gpu_tensor(particles, "particles", promote=True))
        j = u.shape[1]
        c = None if cost is None else L.require_gpu_tensor(cost, "cost", promote=True).contiguous()
        e = torch.empty(j, dtype=torch.float64, device=u.device)
        L.check(
            L.load().pls_onb_prior_energy(self._desc(), u.data_ptr(), L.ld(u), j, L.ptr(c), e.data_ptr(), L.stream_ptr()),
            "pls_onb_prior_energy",
        )
        return e

    def calculate_energy_potential(self, particles: torch.Tensor, cost: torch.Tensor) -> float:
        return _ops.block_means(self.particle_energy_potential(particles, cost)).item()  # :126 (host sync)

    def _calculate_particle_update(self, particles: torch.Tensor, cost_derivative: torch.Tensor, step_size: float,
                                   noise: torch.Tensor | None = None) -> torch.Tensor:
        """dU = -eta V~^T k(Z,X) G - eta Lambda^-1 U + sqrt(2 eta) xi  (:128-159)."""
        u = _rows_contiguous(L.require_gpu_tensor(particles, "particles", promote=True))
        g = _rows_contiguous(L.require_gpu_tensor(cost_derivative, "cost_derivative", promote=True))
        j = u.shape[1]
        assert g.shape == (self._n, j), f"cost_derivative has shape {tuple(g.shape)}, expected ({self._n}, {j})"
        du = torch.empty_like(u, memory_format=torch.contiguous_format)
        nd = self._draw_noise_spec(noise).desc()
        L.check(
            L.load().pls_onb_particle_update(self._desc(), u.data_ptr(), L.ld(u), g.data_ptr(), L.ld(g), j, float(step_size),
                                             nd, du.data_ptr(), L.ld(du), L.stream_ptr()),
            "pls_onb_particle_update",
        )
        return du

    # ---- fused native step ------------------------------------------------------------------------------------------
    def supports_fused_step(self) -> bool:
        return True

    def supports_input_energy(self, cost) -> bool:
        """True if fused_step can return the energy of its input particles as a by-product: every native cost.
        Gaussian/identity: the quadratic form of the same B U product; otherwise the cost VALUE of the same F tile the
        derivative is taken of (the reference recomputes F for the energy: projected_langevin_sampling.py:125-138)."""
        return bool(cost.is_native())

    def supports_energy_sums(self, cost) -> bool:
        """True if the launch that finishes the step's energy by-product can also leave the 256-column chunk sums of the
        energies (BlockSpec.energy_sums): the Gaussian/identity fast path, and every native cost on a basis of at most 128
        functions -- the one-launch small-rank step (pls_block_desc.step_sync) writes them itself, its fall-back for large
        problems appends pls_chunk_sums."""
        return bool(cost.is_native()) and (self._is_gaussian(cost) or self._one_launch_rank(cost))

    def uses_sums16(self, cost) -> bool:
        """True if a training loop should ask for the 16-column sums of the energies (BlockSpec.energy_sums16) instead of the
        256-column chunk sums: the costs whose step is the one-launch small-rank kernel."""
        return bool(cost.is_native()) and self._one_launch_rank(cost)

    def _route(self, cost, j: int, force_generic: bool = False, whitened: bool = False) -> StepRoute:
        """pls_onb_step[_blocks].  The Gaussian/identity fast path takes B = A A^T, c = A y and asks for workspace only for
        the partial rows of its energy by-product (one per 64 data rows); any other cost takes the slab kernels' G chunks
        (or, on a basis of at most 128 functions, the one-launch small-rank step)."""
        assert not whitened, "the orthonormal basis has no whitened coordinates"
        y, cd = cost.y_device(), cost.desc()
        gaussian = self._is_gaussian(cost, force_generic, cd)
        if gaussian:
            self.prepare_gaussian(y)
        desc = self._desc(with_gaussian=gaussian)
        mk = self.approximation_dimension
        wkey = (gaussian, j, self.workspace_bytes)
        ws_bytes = self.__dict__.setdefault("_ws_bytes_cache", {}).get(wkey)
        if ws_bytes is None:
            ws_bytes = self._ws_bytes_cache[wkey] = (self.energy_partial_rows_bytes(j) if gaussian else
                                                     self._general_ws_bytes(L.load().pls_onb_step_workspace_bytes, desc, j))
        planes = None if gaussian else self._winograd_planes(desc)
        entries, tail = ("pls_onb_step", "pls_onb_step_blocks"), (int(force_generic),)
        if planes is not None:  # (the same entries, with the left-hand planes of the Winograd back-projection handed in)
            entries, tail = ("pls_onb_step_wg", "pls_onb_step_blocks_wg"), (*tail, planes.data_ptr(), planes.numel() * 8)
        return StepRoute(*entries, (desc, cd, y.data_ptr()), tail, ws_bytes,
                         (y, self._A, self._At, self.eigenvalues, self._B, self._c, planes),
                         one_launch=not gaussian and 1 <= mk <= self.SMALL_RANK_MAX, sums=gaussian, lagged=gaussian,
                         ws_for_energy_only=gaussian)

    def _winograd_planes(self, desc) -> torch.Tensor | None:
        """The left-hand planes of the general step's Strassen-Winograd back-projection (pls_onb_winograd_prepare), built once
        per projection: None where the route does not apply, and while a graph is being captured (no allocation or setup
        launch inside a capture; that step takes the plain route)."""
        key = self._At.data_ptr()
        cached = self.__dict__.get("_wg_cache")
        if cached is not None and cached[0] == key:
            return cached[1]
        lib = L.load()
        nbytes = int(lib.pls_onb_winograd_bytes(desc))
        planes = None
        if nbytes:
            if torch.cuda.is_current_stream_capturing():
                return None
            planes = torch.empty(nbytes // 8, dtype=torch.float64, device=self._At.device)
            L.check(lib.pls_onb_winograd_prepare(desc, planes.data_ptr(), nbytes, L.stream_ptr()), "pls_onb_winograd_prepare")
            torch.cuda.current_stream(self._At.device).synchronize()  # (steps on any stream read them from here on)
        self._wg_cache = (key, planes)
        return planes

    #: fused_step itself takes BlockSpec.energy_partials (the inducing-point basis only in whitened_step)
    fused_step_takes_lagged_energies = True

    def supports_lagged_energies(self, cost) -> bool:
        """True if a training loop may let launch k + 1 finish the energies of launch k (BlockSpec.energy_partials ...): the
        Gaussian/identity fast path."""
        return bool(cost.is_native()) and self._is_gaussian(cost)

    def energy_partial_rows_bytes(self, j: int) -> int:
        return int(L.load().pls_energy_partials_bytes(self.approximation_dimension, j))

    def eager_step(self, cost, particles: torch.Tensor, step_size: float) -> torch.Tensor | None:
        """dU of one step with the library's own noise for the drop-in loop `particles += pls.calculate_particle_update(...)`
        (README.md:257-262, experiments/profiler/main.py:77-82): fused_step(cost, particles, step_size) through a BoundStep
        cached per (cost, J, step size, stream, targets, ...) -- it owns its workspace, step-size word and counters.  At the
        reference's own benchmark sizes a step is a 5 us kernel, and building the call afresh (~20 us of Python) is what an
        iteration costs.  One draw from torch's global generator per call, like fused_step.  None: not applicable (the
        caller takes fused_step)."""
        if not (particles.is_cuda and particles.dtype == torch.float64 and particles.dim() == 2 and particles.stride(1) == 1):
            return None
        j = particles.shape[1]
        if j == 0:
            return None
        y = cost.y_device()
        key = (id(cost), j, float(step_size), L.stream_ptr(), y.data_ptr(), y._version, getattr(cost, "observation_noise", None),
               self.j_offset, self.workspace_bytes, type(cost), type(cost.link_function), getattr(cost.link_function, "jitter", None))
        cached = self.__dict__.get("_eager")  # (key, BoundStep)
        if cached is None or cached[0] != key:
            cached = self._eager = (key, self._bind_step(cost, particles, step_size, energies=False, new_state=False))
        bound = cached[1]
        seed = int(torch.randint(0, 2**62, (1,), dtype=torch.int64).item())
        out = torch.empty_like(particles, memory_format=torch.contiguous_format)
        ldu = particles.stride(0) if particles.shape[0] > 1 else max(j, particles.stride(0))  # (L.ld, inline: host-bound)
        try:
            bound.launch(particles.data_ptr(), ldu, out.data_ptr(), j, seed)
        except L.PlsHipError:
            self.__dict__.pop("_eager", None)
            raise
        return out

    def flush_energies(self, cost, state: torch.Tensor, blocks: BlockSpec) -> None:
        """Finish the partial rows the LAST step launch of a loop left (``blocks``: energy_flush=True, energy_partials_prev,
        energy_prev[, energy_sums_prev]); ``state``: the particle matrix the step calls were given (same shape / strides)."""
        u = _rows_contiguous(L.require_gpu_tensor(state, "particles"))
        r = self._route(cost, u.shape[1])
        L.check(r.call(blocks.desc(), u.data_ptr(), L.ld(u), u.shape[1], 0.0, NoiseSpec(none=True).desc(), None, 0, L.OUT_DELTA,
                       None, None, 0, L.stream_ptr()), r.blocks_entry)

    def fused_particle_energy(self, cost, particles: torch.Tensor, force_generic: bool = False) -> torch.Tensor:
        """Per-particle energy (pls_onb_energy): the cost is reduced inside a GEMM epilogue -- the N x Mk x J forward
        GEMM in general, the Mk x Mk x J quadratic form for Gaussian/identity."""
        u = _rows_contiguous(L.require_gpu_tensor(particles, "particles", promote=True))
        j = u.shape[1]
        lib = L.load()
        cd = cost.desc()
        gaussian = self._is_gaussian(cost, force_generic, cd)
        if gaussian:
            self.prepare_gaussian(cost.y_device())
        desc = self._desc(with_gaussian=gaussian)
        ws_bytes = min(lib.pls_onb_energy_workspace_bytes(desc, j, self._n), max(self.workspace_bytes, 4 * j * 8))
        ws = self._workspace(ws_bytes, u.device)
        e = torch.empty(j, dtype=torch.float64, device=u.device)
        L.check(
            lib.pls_onb_energy(desc, cd, cost.y_device().data_ptr(), u.data_ptr(), L.ld(u), j, e.data_ptr(),
                               1 if force_generic else 0, ws.data_ptr(), ws_bytes, L.stream_ptr()),
            "pls_onb_energy",
        )
        return e

    # ---- prediction (one-time, not on the step path) -----------------------------------------------
    def sample_predictive_noise(self, particles: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
        """(M_k + N*, J) joint Gaussian noise G([Z, x]) (:161-214).  Gram blocks and the products are libplship kernels, the
        normals come from samplers.DEFAULT_NORMAL_STREAM (the reference's host stream; for a J-sharded run the device generator
        keyed by the global particle column), and
        the (M_k + N*) eigh of the sampler (samplers.py:27) is remembered per test-point tensor: tempering and conformal
        calibration predict at the same points again and again (temper/base.py:30-59, conformalise/base.py:58-114)."""
        lt = self._predictive_factor(x)
        predictive_noise = sample_multivariate_normal(
            mean=torch.zeros(lt.shape[0]), cov=None, size=(particles.shape[1],), factor=lt, j_offset=self.j_offset
        ).T  # :205-209
        if self.additional_predictive_noise_distribution is not None:
            extra = self.additional_predictive_noise_distribution.sample(predictive_noise.shape).reshape(predictive_noise.shape)
            predictive_noise = predictive_noise + _dev(extra)  # :210-213
        return predictive_noise.contiguous()

    def _predictive_covariance(self, x: torch.Tensor) -> torch.Tensor:
        gram_x = self.kernel.forward(x1=x, x2=x, additional_approximation_samples=x)  # r(x,x)  :174-178
        base_gram_induce_x = self.kernel.base_kernel(x1=self.x_induce, x2=x)  # k(Z,x) (M, N*): k-major operand
        # off_diagonal_block = k(x,Z) V~ diag(lambda)  (N*, M_k)  :183-185 -- the column scale is folded into the operand
        off = _ops.gemm_tn(base_gram_induce_x, self._scaled_eigenvectors_lam)
        lam_diag = torch.diag(self.eigenvalues)
        return torch.cat([torch.cat([lam_diag, off.T], dim=1), torch.cat([off, gram_x], dim=1)], dim=0)  # :186-204

    def _predictive_factor(self, x: torch.Tensor) -> torch.Tensor:
        return _cached_factor(self, x, self._predictive_covariance)

    def predict_untransformed_samples(self, particles: torch.Tensor, x: torch.Tensor,
                                      noise: torch.Tensor | None = None) -> torch.Tensor:
        """G(x) + k(x,Z) V~ (U - G(Z))  (:216-244), as  G(x) + P U - P G(Z)  with P^T = V~^T k(Z,x) built once."""
        u = _rows_contiguous(L.require_gpu_tensor(particles, "particles", promote=True))
        base_gram_induce_x = self.kernel.base_kernel(x1=self.x_induce, x2=x)  # k(Z, x) (M, N*)
        if noise is None:
            noise = self.sample_predictive_noise(particles=particles, x=x)
        noise = L.require_gpu_tensor(noise, "noise", promote=True)
        mk = self.approximation_dimension
        pt = _ops.gemm_tn(self.scaled_eigenvectors, base_gram_induce_x)  # (M_k, N*) = V~^T k(Z,x)
        out = noise[mk:, :].contiguous().clone()
        _ops.gemm_tn(pt, u, 1.0, 1.0, out=out)
        _ops.gemm_tn(pt, noise[:mk, :].contiguous(), -1.0, 1.0, out=out)
        return out


#: spectral factors a basis remembers (one per test-point tensor, least recently used out first): tempering and conformal
#: calibration alternate between the calibration points and the test points; an entry is (M_k + N*)^2 doubles
PREDICTIVE_FACTOR_CACHE_ENTRIES = 4


def _cached_factor(basis, x: torch.Tensor, covariance) -> torch.Tensor:
    """spectral_factor(covariance(x)), remembered per test-point tensor: an entry holds a reference to ``x`` (its storage
    cannot be handed to another tensor meanwhile), its version counter (an in-place change rebuilds) and the eigh default in
    force when it was built."""
    from .. import samplers

    key = (x._version, tuple(x.shape), samplers.DEFAULT_EIGH_DEVICE)
    cache = basis.__dict__.setdefault("_pred_factor_cache", [])
    for i, (xr, k, lt) in enumerate(cache):
        if xr is x and k == key:
            cache.append(cache.pop(i))
            return lt
    cache[:] = [e for e in cache if e[0] is not x]  # (a stale entry of the same tensor)
    lt = samplers.spectral_factor(covariance(x))
    cache.append((x, key, lt))
    del cache[:-PREDICTIVE_FACTOR_CACHE_ENTRIES]
    return lt

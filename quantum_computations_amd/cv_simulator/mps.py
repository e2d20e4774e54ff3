"""Register of the CV simulator behind the reference's ``MPS`` surface, in HBM, in one of two layouts.

``layout="sites"`` (default) is the reference's own data structure -- a chain of ``(chi_l, d, chi_r)`` site tensors
(``simulators/cv_simulator/mps.py:102-201``) re-compressed with a truncated SVD after every two-mode gate -- kept on the
device by ``site_register.SiteRegister``; this is what reaches the reference's d = 1000 grids, what
honours the truncation keywords, and what a script written for the reference gets when it calls ``MPS(qs, tensors)``.

``layout="dense"`` (opt-in) holds the *contracted* tensor ``psi[q_0, ..., q_{m-1}]`` as a ``QuditState``
(``d = len(domain)`` levels per mode): every gate is one bandwidth-bound pass, results equal the reference's with
truncation disabled (``rel_err = 0``), truncation keywords are ignored, and the size is limited by ``d^m * 16`` bytes
(the Fock-truncated configuration of BASELINE.json, ``cv_simulator.fock``, is this kind of register).

Either way the class keeps the constructor, ``domain`` / ``diff``, ``len``, ``copy``, ``validate``, ``contract``,
``norm`` and ``partial_density_mps`` of the reference class, and the gate classes drive both through the same calls.
"""
from __future__ import annotations

import inspect
import logging
from functools import reduce

import numpy as np

from ..device import QuditState


def tensor_svd(tensor, left_indices, right_indices, *, max_bond_dim: int = np.inf, abs_err: float = 0,
               rel_err: float = 1e-12, rng_seed: int = None, device: int = 0):
    """Split a host tensor by a truncated SVD on the device (``tensor_svd``, mps.py:52-97): returns ``m1`` with legs
    ``left_indices + [j]`` and ``m2`` with legs ``[j] + right_indices``; the singular values are shared as square
    roots and the kept rank follows the reference's rule (tail sum <= max(abs_err, rel_err * sum), then the cap)."""
    from .site_register import SiteRegister
    left_indices, right_indices = list(left_indices), list(right_indices)
    if sorted(left_indices + right_indices) != list(range(np.ndim(tensor))):
        raise IndexError("Output indices does not match indices of initial tensor")
    shape = np.shape(tensor)
    rows = int(np.prod([shape[i] for i in left_indices]))
    cols = int(np.prod([shape[i] for i in right_indices]))
    matrix = np.moveaxis(np.asarray(tensor), left_indices + right_indices, range(len(shape))).reshape(rows, cols)
    worker = SiteRegister([], 1, device)
    m1, m2, r = worker._split(worker._upload(matrix), rows, cols, max_bond_dim=max_bond_dim, abs_err=abs_err,
                              rel_err=rel_err, rng_seed=rng_seed)
    return (m1.cpu().numpy().reshape([shape[i] for i in left_indices] + [r]),
            m2.cpu().numpy().reshape([r] + [shape[i] for i in right_indices]))


# the keyword-only truncation options gates and the simulator accept (mps.py:99-100)
SVD_OPTIONS = {name: p for name, p in inspect.signature(tensor_svd).parameters.items()
               if p.kind == inspect.Parameter.KEYWORD_ONLY}


class MPS:
    def __init__(self, domain: np.ndarray, tensors: list[np.ndarray], *, device: int = 0, layout: str = "sites"):
        """``tensors``: one entry per mode -- a wavefunction on ``domain`` (1-D) or an MPS site ``(chi_l, d, chi_r)``.
        ``layout="sites"`` (the reference's behaviour): the sites are uploaded as they are and stay a matrix-product
        state; ``layout="dense"``: the sites are contracted on the host (small registers) and the dense tensor is
        uploaded."""
        if layout not in ("dense", "sites"):
            raise ValueError("layout must be 'dense' or 'sites'")
        self.domain: np.ndarray = domain
        self._check_domain()
        self.diff: float = abs(domain[-1] - domain[0]) / (len(domain) - 1)
        sites = [np.asarray(t).reshape(1, -1, 1) if np.ndim(t) == 1 else np.asarray(t) for t in tensors]
        self._check_sites(sites)
        d = len(domain)
        if layout == "sites":
            from .site_register import SiteRegister
            self.reg = SiteRegister(sites, d, device)
        elif sites:
            dense = np.squeeze(reduce(lambda a, b: np.tensordot(a, b, axes=1), sites), axis=(0, -1))
            self.reg = QuditState.from_numpy(np.ascontiguousarray(dense, dtype=np.complex128).reshape((d,) * len(sites)),
                                             device)
        else:
            self.reg = QuditState.zeros(0, d, device)

    @classmethod
    def _wrap(cls, domain: np.ndarray, reg: QuditState) -> "MPS":
        out = cls.__new__(cls)
        out.domain = domain
        out.diff = abs(domain[-1] - domain[0]) / (len(domain) - 1)
        out.reg = reg
        return out

    # ---- container protocol (the reference class is a list of site tensors, mps.py:102-134) ----------
    def __len__(self):
        return self.reg.dims[0]

    def _sites_only(self, what: str):
        if self.layout != "sites":
            raise AttributeError(f"a dense register has no site tensors ({what}): build the MPS with layout='sites'")

    def __getitem__(self, index):
        """Host copy of site ``index`` (or of a slice of sites)."""
        self._sites_only("indexing")
        picked = self.reg.sites[index]
        with self.reg.stream_context():
            return [t.cpu().numpy() for t in picked] if isinstance(index, slice) else picked.cpu().numpy()

    def __setitem__(self, index: int, tensor: np.ndarray) -> None:
        """Replace site ``index`` (uploaded; shapes are the caller's responsibility until :meth:`validate`)."""
        self._sites_only("item assignment")
        tensor = np.asarray(tensor)
        if tensor.ndim != 3:
            raise ValueError(f"Tensor at index {index} does not have exactly three axes.")
        self.reg.sites[index] = self.reg._upload(tensor)

    def __iter__(self):
        self._sites_only("iteration")
        return iter(self.reg.site_arrays())

    def copy(self) -> "MPS":
        return MPS._wrap(self.domain.copy(), self.reg.copy())

    @property
    def layout(self) -> str:
        return getattr(self.reg, "layout", "dense")

    @property
    def tensors(self) -> list[np.ndarray]:
        """Host copies of the site tensors (``layout="sites"`` only; the dense register has no sites)."""
        self._sites_only("tensors")
        return self.reg.site_arrays()

    def shape(self):
        if self.layout == "sites":
            return self.reg.shape()
        n, d = self.reg.dims
        return ("dense",) + (d,) * n

    # ---- validation (mps.py:136-161) ----------------------------------------------------------------
    def _check_domain(self):
        if not isinstance(self.domain, np.ndarray) or self.domain.ndim != 1:
            raise TypeError("Domain must be a 1D numpy array.")
        if not np.allclose(np.diff(self.domain, 2), 0, atol=np.finfo(self.domain.dtype).eps ** 0.5):
            raise ValueError("Domain is not an arithmetic progression.")

    def _check_sites(self, sites):
        for idx, t in enumerate(sites):
            if t.ndim != 3:
                raise ValueError(f"Tensor at index {idx} does not have exactly three axes.")
            if t.shape[1] != len(self.domain):
                raise ValueError(f"Tensor at index {idx} does not have the right physical dimension.")
        if sites:
            if sites[0].shape[0] != 1:
                raise ValueError("Left-most tensor does not have a trivial left edge")
            if sites[-1].shape[2] != 1:
                raise ValueError("Right-most tensor does not have a trivial right edge")
        for idx, (a, b) in enumerate(zip(sites, sites[1:])):
            if a.shape[2] != b.shape[0]:
                raise ValueError(f"Tensors at indices {idx} and {idx + 1} do not have compatible bond dimensions.")

    def validate(self):
        self._check_domain()
        if not np.isclose(self.diff, abs(self.domain[-1] - self.domain[0]) / (len(self.domain) - 1)):
            raise ValueError("Stored difference does not match current domain.")
        if self.reg.dims[1] != len(self.domain):
            raise ValueError("Register does not have the right physical dimension.")

    # ---- read-out ---------------------------------------------------------------------------------------
    def contract(self) -> np.ndarray:
        """The dense tensor ``psi[q_0, ..., q_{m-1}]`` on the host (``MPS.contract``, mps.py:163-164)."""
        return self.reg.to_numpy()

    def norm(self) -> float:
        """``sqrt(int |psi|^2)`` with the grid measure ``diff^m`` (mps.py:166-170)."""
        return float(np.sqrt(self.reg.norm2() * self.diff ** len(self)))

    def marginal(self, axis: int) -> np.ndarray:
        """Diagonal of :meth:`partial_density_mps` -- the position density of mode ``axis`` -- computed on the device."""
        if axis < 0 or axis >= len(self):
            raise IndexError(f"axis={axis} out of bounds")
        return self.reg.marginal(axis) * self.diff ** (len(self) - 1)

    def partial_density_mps(self, axis: int) -> np.ndarray:
        """Reduced density matrix of mode ``axis`` (mps.py:176-190).  Host contraction of the downloaded tensor:
        for read-out of small registers; measurements use :meth:`marginal`, which stays on the GPU."""
        if axis < 0 or axis >= len(self):
            raise IndexError(f"axis={axis} out of bounds")
        if self.layout == "sites":
            return self.reg.reduced_density(axis) * self.diff ** (len(self) - 1)
        psi = np.moveaxis(self.contract(), axis, 0).reshape(len(self.domain), -1)
        return (psi @ psi.conj().T) * self.diff ** (len(self) - 1)

    def wigner(self, mode, q, p, *, normalised: bool = False) -> np.ndarray:
        """Wigner function of the reduced state of ``mode`` on the window ``q x p`` (hbar = 1), shape ``(len(p), len(q))``
        -- the orientation of ``contourf(*np.meshgrid(q, p), W)``.  A sequence of modes gives ``(len(modes), len(p),
        len(q))`` from one batched launch.  The density matrices carry the grid measure ``diff^(m-1)`` of
        :meth:`partial_density_mps`, so the integral of ``W`` is ``norm()**2`` unless ``normalised`` divides by it.

        ``layout="sites"``: the reduced density matrices are contracted on the device
        (``SiteRegister.reduced_density_device``) and never leave it.  ``layout="dense"``: they are built on the host by
        :meth:`partial_density_mps` and uploaded."""
        from .utils import wigner_device
        modes = [mode] if np.ndim(mode) == 0 else list(mode)
        for axis in modes:
            if int(axis) != axis or axis < 0 or axis >= len(self):
                raise IndexError(f"mode={axis} out of bounds")
        modes = [int(axis) for axis in modes]
        if self.layout == "sites":
            rho = self.reg.reduced_density_device(modes)
            with self.reg.stream_context():
                w = wigner_device(rho, self.domain, q, p, normalised=normalised)
            if not normalised:
                w *= self.diff ** (len(self) - 1)
        else:
            from .site_register import _torch
            torch = _torch()
            host = np.stack([self.partial_density_mps(axis) for axis in modes])
            rho = torch.from_numpy(np.ascontiguousarray(host, dtype=np.complex128)).to(torch.device("cuda", int(self.reg.device)))
            w = wigner_device(rho, self.domain, q, p, normalised=normalised)
        return w if np.ndim(mode) else w[0]

    def sample(self, shots: int, *, quadratures=None, rng=None, return_density: bool = False):
        """``shots`` independent outcomes of measuring every mode, as grid values ``(shots, m)``; the register is not
        modified.  Shot ``s`` is what the chain ``Mq(0), Mq(0), ...`` (gates.py:87-117) returns on a copy of the register
        when ``rng.choice`` is fed ``U[s, :]`` of ``U = rng.random((shots, m))``; all shots advance through the chain
        together on the device (``SiteRegister.sample``).  No upstream counterpart.

        ``quadratures[k]``: ``"q"`` (default), ``"p"`` (the inverse Fourier matrix of ``Mp``) or an angle (the rotation
        by ``-angle`` of ``Homodyne``; multiples of pi measure ``q`` and multiply the outcome by ``round(cos(angle))``).
        ``rng``: a ``numpy.random.Generator`` or a seed.  ``return_density=True`` also returns the probability density
        of every outcome given the shot's earlier ones (``MeasurementResult.probability``), ``(shots, m)``: the product
        along a row is the joint density of the shot."""
        from .utils import fourier_matrix, rotation_matrix
        self._sites_only("sampling")
        m = len(self)
        if int(shots) != shots or shots < 1:
            raise ValueError(f"shots must be a positive integer, got {shots}")
        if m < 1:
            raise IndexError("cannot sample an empty register")
        quadratures = ["q"] * m if quadratures is None else list(quadratures)
        if len(quadratures) != m:
            raise IndexError(f"quadratures must have one entry per mode ({m}), got {len(quadratures)}")
        built: dict = {}
        operators, signs = [None] * m, np.ones(m)
        for k, quad in enumerate(quadratures):
            if isinstance(quad, str):
                if quad not in ("q", "p"):
                    raise ValueError(f"quadratures[{k}] must be 'q', 'p' or an angle, got {quad!r}")
                if quad == "p":
                    if "p" not in built:
                        built["p"] = fourier_matrix(self.domain, inv=True)
                    operators[k] = built["p"]
                continue
            angle = float(quad)
            if np.isclose(np.sin(angle), 0):
                signs[k] = np.round(np.cos(angle))
                continue
            if angle not in built:
                built[angle] = rotation_matrix(self.domain, -angle)
            operators[k] = built[angle]
        generator = rng if isinstance(rng, np.random.Generator) else np.random.default_rng(rng)
        uniforms = generator.random((int(shots), m))
        picks, densities = self.reg.sample(uniforms, operators if any(op is not None for op in operators) else None,
                                           measure=self.diff)
        if not np.all(np.isfinite(densities)) or np.any(densities <= 0):
            raise ValueError("sampling met an outcome of zero density: the register has no norm")
        values = self.domain[picks] * signs
        return (values, densities) if return_density else values

    # ---- canonical forms, Schmidt spectra, compression (no upstream counterpart) ------------------------------------
    def canonicalise(self, centre: int = 0, *, rank_tol: float = 1e-13) -> list[np.ndarray]:
        """Mixed canonical form around ``centre``, in place (``SiteRegister.canonicalise``): sites before ``centre`` become
        left isometries, sites after it right isometries, the state stays what it was up to rounding.  Returns the Schmidt
        values of all ``m - 1`` bonds (of the unnormalised state, without grid-measure factors)."""
        self._sites_only("canonicalise")
        return self.reg.canonicalise(centre, rank_tol)

    def compress(self, centre: int = 0, **svd_options) -> list[float]:
        """Truncate every bond of the finished register by its Schmidt values with the rule of the gates'
        ``max_bond_dim`` / ``abs_err`` / ``rel_err`` (``SiteRegister.compress``), in place; returns the discarded weight
        per bond relative to ``norm()**2``.  Unknown keywords are logged and ignored, like the gates do."""
        self._sites_only("compress")
        known = {k: v for k, v in svd_options.items() if k in ("max_bond_dim", "abs_err", "rel_err")}
        for name in svd_options:
            if name not in known:
                logging.getLogger(__name__).warning("compress ignores the keyword %r", name)
        return self.reg.compress(centre, **known)

    def schmidt_values(self, bond: int | None = None):
        """Schmidt values of the cut between modes ``bond`` and ``bond + 1`` (or the list for all ``m - 1`` cuts),
        computed on a canonicalised copy: the register is untouched."""
        self._sites_only("schmidt_values")
        m = len(self)
        if bond is not None and (int(bond) != bond or not 0 <= bond < m - 1):
            raise IndexError(f"bond={bond} out of bounds for {m} modes")
        if m < 1:
            raise IndexError("an empty register has no bonds")
        work = self.reg.copy()
        values = work.canonicalise(0)
        work.sites = []
        return values if bond is None else values[int(bond)]

    def entanglement_entropy(self, bond: int | None = None):
        """Von Neumann entropy (nats) of ``p = s^2 / sum s^2`` over the Schmidt values of ``bond`` (or of every bond)."""
        values = self.schmidt_values(bond)

        def entropy(s):
            p = np.asarray(s, dtype=np.float64) ** 2
            p = p[p > 0] / np.sum(p)
            return float(-np.sum(p * np.log(p)))

        return entropy(values) if bond is not None else [entropy(s) for s in values]

    @staticmethod
    def overlap(a: "MPS", b: "MPS") -> complex:
        """``<a|b> = int conj(a) b`` with the grid measure ``diff^m``, contracted site by site on the device
        (``SiteRegister.overlap``): no dense tensor is built."""
        a._sites_only("overlap")
        b._sites_only("overlap")
        if len(a) != len(b):
            raise ValueError("registers of different sizes")
        if len(a.domain) != len(b.domain) or not np.allclose(a.domain, b.domain):
            raise ValueError("registers on different grids")
        if a.reg.device != b.reg.device:
            raise ValueError("registers on different devices")
        return a.reg.overlap(b.reg) * a.diff ** len(a)

    @staticmethod
    def fidelity(a: "MPS", b: "MPS") -> float:
        """``|<a|b>|^2`` on a shared grid.  (The reference's version, mps.py:192-201, contracts ``a`` with itself
        and never reads ``b``; this one computes what its docstring says.)  Two ``sites`` registers go through
        :meth:`overlap` and need no ``d^m`` host memory; a dense register is contracted on the host."""
        if len(a) != len(b):
            raise ValueError("registers of different sizes")
        if a.layout == "sites" and b.layout == "sites":
            return float(np.abs(MPS.overlap(a, b)) ** 2)
        overlap = np.vdot(a.contract(), b.contract()) * a.diff ** len(a)
        return float(np.abs(overlap) ** 2)

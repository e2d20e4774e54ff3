"""Matrix-product-state register of the CV simulator, resident in HBM.

The reference keeps a CV state as a list of ``(chi_l, d, chi_r)`` site tensors (``simulators/cv_simulator/mps.py:102-201``)
and re-compresses after every two-mode gate: contract the two neighbours, map the ``(q_left, q_right)`` plane, split with
a truncated SVD (``cv_simulator/gates.py:48-84,151-192``).  ``SiteRegister`` is that data structure with every tensor in
device memory and every step done by libqsv.so on the GPU:

====================================  ==========================================================================
step                                  entry point
====================================  ==========================================================================
single-mode operator on a site        ``qsv_tensor_apply_axis_dev`` (rocBLAS zgemm for grids >= 64 points)
single-mode phases (Z, P)             ``qsv_tensor_scale_axis``
theta = site_l . site_r               ``qsv_tensor_gemm``
CZ phases / BS, CX resampling / SWAP   ``qsv_tensor_plane_phase`` / ``qsv_tensor_plane_affine`` / ``qsv_tensor_plane_gather``
split + truncate                      ``qsv_tensor_svd_split`` / ``qsv_tensor_rsvd_split`` (rocSOLVER + the reference's rule)
homodyne read-out                     ``qsv_tensor_gemm`` environments + ``qsv_tensor_axis_overlap``; ``qsv_tensor_take_level``
Insert in the middle of the chain     ``qsv_tensor_insert_axis`` + ``qsv_tensor_svd_split``
====================================  ==========================================================================

PyTorch only owns the device buffers (allocation, host<->device copies, the current stream); no torch operator touches
the amplitudes.  The interface is the one ``QuditState`` offers the gate classes, so ``cv_simulator.gates`` drive either
register; the truncation keywords of the gates (``max_bond_dim``, ``abs_err``, ``rel_err``) arrive as keyword arguments.

Like the reference, the split is exact (rocSOLVER ``zgesvd``) unless ``max_bond_dim * 10 < min(matrix shape)``, where it
switches to the randomized range finder of ``mps.py:5-50`` (``qsv_tensor_rsvd_split``: GEMMs + Householder QR + a small
SVD), fed with the same Gaussian test matrix a seeded reference run would draw.

A register works on torch's current stream unless it is given one (``stream=`` or :meth:`SiteRegister.adopt_stream`);
then every launch, allocation and wait of the register goes to that stream, so that independent registers run side by
side on their own streams (``quantum_computations_amd.concurrent``).
"""
from __future__ import annotations

import contextlib
import ctypes as C
import functools
from collections import OrderedDict
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from .. import _lib

OP_NONE, OP_TRANSPOSE, OP_CONJ_TRANSPOSE = 0, 1, 2


def kept_rank(s, max_bond_dim=np.inf, abs_err: float = 0, rel_err: float = 1e-12) -> int:
    """How many of the decreasing values ``s`` the truncation rule of the splits keeps (``tensor_svd``, mps.py:86-93;
    ``qsv_tensor_svd_split``): drop the longest tail whose sum stays ``<= max(abs_err, rel_err * sum(s))``, then cap at
    ``max_bond_dim``; at least one value stays."""
    s = np.asarray(s, dtype=np.float64)
    tails = np.cumsum(s[::-1])[::-1]                    # tails[i] = s[i] + ... + s[-1]
    keep = int(np.count_nonzero(tails > max(abs_err, rel_err * float(np.sum(s)))))
    if np.isfinite(max_bond_dim):
        keep = min(keep, int(max_bond_dim))
    return max(1, keep)


_TORCH = None


def _torch():
    """The torch module, after checking once that a HIP device is there (buffers only: allocation, copies, streams)."""
    global _TORCH
    if _TORCH is None:
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("SiteRegister needs a HIP device: there is no CPU fallback")
        _TORCH = torch
    return _TORCH


def _on_stream(method):
    """Run ``method`` with the register's own stream as torch's current stream (when it has one), so that torch's
    allocations, copies and read-backs are ordered with the register's launches."""
    @functools.wraps(method)
    def wrapper(self, *args, **kwargs):
        if self.stream is None:
            return method(self, *args, **kwargs)
        with self.stream_context():
            return method(self, *args, **kwargs)
    return wrapper


class SiteRegister:
    layout = "sites"

    def __init__(self, sites: list[np.ndarray], d: int, device: int = 0, stream=None):
        """``stream``: a ``torch.cuda.Stream`` of ``device`` this register works on; None = torch's current stream at
        each call (the default)."""
        torch = _torch()
        self.device = int(device)
        self._dev = torch.device("cuda", self.device)
        self.d = int(d)
        self.stream = stream
        self._draw_pool: ThreadPoolExecutor | None = None            # see _split: one helper thread per register
        self.sites = [self._upload(np.asarray(s).reshape(1, -1, 1) if np.ndim(s) == 1 else s) for s in sites]
        self._resident: OrderedDict[int, tuple] = OrderedDict()    # host operator id -> (host array, device copy)
        self._scratch_buffers: dict = {}
        self.last_singular_values: np.ndarray | None = None
        self.split_counts = {"exact": 0, "randomized": 0}          # which branch of tensor_svd the splits took

    # ---- plumbing ----------------------------------------------------------------------------------------
    @_on_stream
    def _upload(self, array, dtype=np.complex128):
        torch = _torch()
        host = np.ascontiguousarray(array, dtype=dtype)
        if not host.flags.writeable:
            host = host.copy()          # torch.from_numpy insists on a writable buffer (cached read-only operators)
        return torch.from_numpy(host).to(self._dev)

    @_on_stream
    def _empty(self, *shape):
        torch = _torch()
        return torch.empty(shape, dtype=torch.complex128, device=self._dev)

    @_on_stream
    def _scratch(self, slot: str, *shape):
        """A complex128 tensor of ``shape`` carved from this register's persistent scratch buffer ``slot`` (grow-only).
        The two-site temporaries (theta, its mapped image, the capacity-sized split outputs) are gigabytes at the
        reference's sizes and die within the gate: re-using one buffer per role keeps hipMalloc / hipFree -- which
        synchronise the device -- out of the gate loop."""
        torch = _torch()
        count = int(np.prod(shape))
        held = self._scratch_buffers.get(slot)
        if held is None or held.numel() < count:
            self._scratch_buffers.pop(slot, None)
            held = torch.empty(count + count // 8, dtype=torch.complex128, device=self._dev)
            self._scratch_buffers[slot] = held
        return held[:count].view(*shape)

    def stream_context(self):
        """Context manager that makes the register's stream torch's current one (nothing to do without one)."""
        return _torch().cuda.stream(self.stream) if self.stream is not None else contextlib.nullcontext()

    def _torch_stream(self):
        return self.stream if self.stream is not None else _torch().cuda.current_stream(self._dev)

    def _stream(self) -> C.c_void_p:
        return C.c_void_p(self._torch_stream().cuda_stream)

    def _keep(self, host: np.ndarray, dtype=np.complex128):
        """Device copy of a host operator, cached while the caller keeps handing in the same array object."""
        key = id(host)
        hit = self._resident.get(key)
        if hit is not None and hit[0] is host:
            self._resident.move_to_end(key)
            return hit[1]
        dev = self._upload(host, dtype)
        self._resident[key] = (host, dev)
        while len(self._resident) > 16:
            self._resident.popitem(last=False)
        return dev

    @staticmethod
    def _p(t) -> C.c_void_p:
        return C.c_void_p(t.data_ptr())

    def _gemm(self, a, op_a: int, b, op_b: int, m: int, n: int, k: int, scratch: str | None = None):
        out = self._scratch(scratch, m, n) if scratch else self._empty(m, n)
        _lib.call("qsv_tensor_gemm", self.device, self._stream(), op_a, op_b, m, n, k, self._p(a), self._p(b),
                  self._p(out))
        return out

    # ---- register protocol shared with QuditState -----------------------------------------------------------
    @property
    def dims(self) -> tuple[int, int]:
        return len(self.sites), self.d

    def bond_dims(self) -> list[int]:
        return [int(s.shape[2]) for s in self.sites[:-1]]

    def shape(self):
        return tuple(tuple(int(x) for x in s.shape) for s in self.sites)

    def sync(self) -> None:
        """Wait for the register's stream (not the whole device: other registers may be working on theirs)."""
        self._torch_stream().synchronize()

    def close(self) -> None:
        """Drop the site tensors and give the library's scratch memory back: the context of the register's own stream
        when it has one (other streams keep working), otherwise every context of the device."""
        self.sites = []
        self._resident.clear()
        self._scratch_buffers.clear()
        if self._draw_pool is not None:
            self._draw_pool.shutdown(wait=True)
            self._draw_pool = None
        if self.stream is not None:
            _lib.call("qsv_tensor_release_stream_workspace", self.device, self._stream())
        else:
            _lib.call("qsv_tensor_release_workspace", self.device)

    def adopt_stream(self, stream, source=None) -> None:
        """Move the register to ``stream`` (e.g. built by ``parse_to_mps`` on the main thread, run on a worker's stream).
        ``stream`` waits for what is queued on ``source`` -- the stream the register's tensors were made on; default:
        the register's own stream, or torch's current stream of the calling thread -- and every device tensor the
        register holds is marked as used on ``stream``: otherwise torch's caching allocator could hand a freed site's
        block back to ``source`` while ``stream`` still reads it.  From then on the register owns ``stream``: ``close``
        releases that stream's library context only."""
        torch = _torch()
        old = source if source is not None else self._torch_stream()
        if stream != old:
            ready = torch.cuda.Event()
            ready.record(old)
            stream.wait_event(ready)
            held = list(self.sites) + list(self._scratch_buffers.values()) + [dev for _, dev in self._resident.values()]
            for t in held:
                t.record_stream(stream)
        self.stream = stream

    @_on_stream
    def copy(self) -> "SiteRegister":
        out = SiteRegister([], self.d, self.device, stream=self.stream)
        out.sites = [s.clone() for s in self.sites]     # device-to-device copies
        return out

    @_on_stream
    def site_arrays(self) -> list[np.ndarray]:
        """The site tensors on the host (``MPS.tensors`` of the reference)."""
        return [s.cpu().numpy() for s in self.sites]

    @_on_stream
    def to_numpy(self) -> np.ndarray:
        """Contract the chain on the device (``MPS.contract``, mps.py:163-164) and download ``psi[q_0, ..., q_{m-1}]``."""
        if not self.sites:
            return np.ones((), dtype=np.complex128)
        acc = self.sites[0]
        rows = int(acc.shape[0] * acc.shape[1])
        for site in self.sites[1:]:
            chi, cols = int(site.shape[0]), int(site.shape[1] * site.shape[2])
            acc = self._gemm(acc, OP_NONE, site, OP_NONE, rows, cols, chi)
            rows = rows * self.d
        return acc.cpu().numpy().reshape((self.d,) * len(self.sites))

    # ---- environments (mps.py:166-190) ------------------------------------------------------------------------
    def _left_environment(self, stop: int):
        """conj of ``reduce("ab,aci,bcj -> ij")`` over the sites before ``stop`` (the conjugate is what chains through
        GEMMs with a conjugate-transposed first operand: X = G^H T, G' = X^H T)."""
        g = self._upload(np.ones((1, 1)))
        for t in self.sites[:stop]:
            cl, d, cr = (int(x) for x in t.shape)
            x = self._gemm(g, OP_CONJ_TRANSPOSE, t, OP_NONE, cl, d * cr, cl)          # X[b, (c, i)]
            g = self._gemm(x, OP_CONJ_TRANSPOSE, t, OP_NONE, cr, cr, cl * d)          # conj(res')[i, j]
        return g

    def _right_environment(self, start: int):
        """``reduce("ica,jcb,ab -> ij")`` over the sites after ``start``, from the right end."""
        r = self._upload(np.ones((1, 1)))
        for t in reversed(self.sites[start + 1:]):
            cl, d, cr = (int(x) for x in t.shape)
            y = self._gemm(t, OP_NONE, r, OP_NONE, cl * d, cr, cr)                    # Y[(i, c), b]
            r = self._gemm(y, OP_NONE, t, OP_CONJ_TRANSPOSE, cl, cl, d * cr)          # right'[i, j]
        return r

    @_on_stream
    def norm2(self) -> float:
        g = self._left_environment(len(self.sites))
        return float(g.cpu().numpy()[0, 0].real)

    def _dressed_site(self, axis: int):
        """``Z[b, i, d] = sum_{a, c} left[a, b] t[a, i, c] right[c, d]`` for the site at ``axis``."""
        t = self.sites[axis]
        cl, d, cr = (int(x) for x in t.shape)
        g, r = self._left_environment(axis), self._right_environment(axis)
        w = self._gemm(t, OP_NONE, r, OP_NONE, cl * d, cr, cr)
        return self._gemm(g, OP_CONJ_TRANSPOSE, w, OP_NONE, cl, d * cr, cl), t

    @_on_stream
    def marginal(self, axis: int) -> np.ndarray:
        """``sum over the other modes of |psi|^2`` per grid point of mode ``axis`` (no grid-measure factors)."""
        torch = _torch()
        z, t = self._dressed_site(axis)
        cl, d, cr = (int(x) for x in t.shape)
        out = torch.empty(d, dtype=torch.float64, device=self._dev)
        _lib.call("qsv_tensor_axis_overlap", self.device, self._stream(), self._p(z), self._p(t), cl, d, cr, self._p(out))
        return out.cpu().numpy()

    @_on_stream
    def reduced_density(self, axis: int) -> np.ndarray:
        """Full ``(d, d)`` reduced density matrix (mps.py:176-190): environments on the device, the last small
        contraction on the host."""
        z, t = self._dressed_site(axis)
        host_t = t.cpu().numpy()
        return np.einsum("bid,bjd -> ij", z.cpu().numpy().reshape(host_t.shape), np.conj(host_t), optimize=True)

    @_on_stream
    def reduced_density_device(self, axes) -> "torch.Tensor":
        """Reduced density matrices of the sites ``axes`` as one device tensor ``(len(axes), d, d)`` (no grid-measure
        factors): :meth:`reduced_density` with the last contraction on the GPU too (``qsv_tensor_axis_density``: the
        physical index moved to the front of the dressed site and of its conjugate, then one GEMM), so no site tensor
        leaves the device."""
        axes = [int(a) for a in axes]
        out = self._empty(len(axes), self.d, self.d)
        for slot, axis in enumerate(axes):
            z, t = self._dressed_site(axis)
            cl, d, cr = (int(x) for x in t.shape)
            _lib.call("qsv_tensor_axis_density", self.device, self._stream(), self._p(z), self._p(t), cl, d, cr,
                      self._p(out[slot]))
        return out

    # ---- canonical forms (no upstream counterpart) --------------------------------------------------------------
    def _orthogonalise(self, site, side: int, rank_tol: float):
        """``qsv_tensor_site_orthogonalise`` of one site: ``(iso, carry, singular values)`` with compact device
        tensors -- ``iso`` ``(L, d, r)`` and ``carry`` ``(r, R)`` for ``side = 0``, ``carry`` ``(L, r)`` and ``iso``
        ``(r, d, R)`` for ``side = 1``."""
        cl, d, cr = (int(x) for x in site.shape)
        width = cr if side == 0 else cl
        rows, cols = (cl * d, cr) if side == 0 else (cl, d * cr)
        iso, carry = self._scratch("iso", cl * d * cr), self._scratch("carry", width * width)
        s = np.zeros(min(rows, cols), dtype=np.float64)
        rank = C.c_uint64(0)
        _lib.call("qsv_tensor_site_orthogonalise", self.device, self._stream(), self._p(site), cl, d, cr, int(side),
                  float(rank_tol), self._p(iso), self._p(carry), C.byref(rank), s.ctypes.data_as(C.c_void_p))
        r = int(rank.value)
        if r < 1:
            raise ValueError("cannot orthogonalise a site that is zero: the register has no norm")
        if side == 0:
            return iso[: cl * d * r].view(cl, d, r), carry[: r * cr].view(r, cr), s
        return iso[: r * d * cr].view(r, d, cr), carry[: cl * r].view(cl, r), s

    def _check_centre(self, centre) -> int:
        m = len(self.sites)
        if m < 1:
            raise IndexError("cannot canonicalise an empty register")
        if int(centre) != centre or not 0 <= centre < m:
            raise IndexError(f"centre={centre} out of bounds for {m} modes")
        return int(centre)

    def _sweep_right(self, stop: int, rank_tol: float) -> None:
        """Make the sites before ``stop`` left isometries, each carry absorbed into its right neighbour."""
        for k in range(stop):
            iso, carry, _ = self._orthogonalise(self.sites[k], 0, rank_tol)
            r = int(carry.shape[0])
            nb = self.sites[k + 1]
            _, d, ncr = (int(x) for x in nb.shape)
            self.sites[k] = iso.clone()
            self.sites[k + 1] = self._gemm(carry, OP_NONE, nb, OP_NONE, r, d * ncr, int(carry.shape[1])).reshape(r, d, ncr)

    def _sweep_left(self, stop: int, rank_tol: float, keep=None) -> list[np.ndarray]:
        """Make the sites after ``stop`` right isometries from the right end, each carry absorbed into its left
        neighbour; returns the singular values met at the bonds ``m - 2, ..., stop`` in that order.  ``keep(s)`` = how
        many of them stay (default: all the library kept)."""
        met = []
        for k in range(len(self.sites) - 1, stop, -1):
            iso, carry, s = self._orthogonalise(self.sites[k], 1, rank_tol)
            r = int(iso.shape[0])
            s = s[:r].copy()
            met.append(s)
            cut = r if keep is None else max(1, min(r, int(keep(s))))
            _, d, cr = (int(x) for x in iso.shape)
            self.sites[k] = iso[:cut].clone()
            if cut < r:
                carry = carry[:, :cut].contiguous()
            nb = self.sites[k - 1]
            ncl, nd, chi = (int(x) for x in nb.shape)
            self.sites[k - 1] = self._gemm(nb, OP_NONE, carry, OP_NONE, ncl * nd, cut, chi).reshape(ncl, nd, cut)
        return met

    @_on_stream
    def canonicalise(self, centre: int, rank_tol: float = 1e-13) -> list[np.ndarray]:
        """Bring the register into mixed canonical form around ``centre``, in place: the sites before ``centre`` become
        left isometries (``sum_{l,j} conj(A[l,j,r]) A[l,j,r'] = 1``), the sites after it right isometries, and the state
        is unchanged up to rounding.  The sweep runs all the way to the right end, back to site 0 and forward again to
        ``centre``: the way back meets every bond with orthonormal environments on both sides, so the singular values
        it finds are the Schmidt values of the state.  They are returned for all ``m - 1`` bonds (bond ``b`` joins
        sites ``b`` and ``b + 1``).  Bonds shrink to their numerical rank: Schmidt values at or below
        ``rank_tol * s[0]`` are dropped."""
        centre = self._check_centre(centre)
        if not (np.isfinite(rank_tol) and rank_tol >= 0):
            raise ValueError(f"rank_tol must be finite and >= 0, got {rank_tol}")
        m = len(self.sites)
        self._sweep_right(m - 1, rank_tol)
        schmidt = self._sweep_left(0, rank_tol)[::-1]
        self._sweep_right(centre, rank_tol)
        return schmidt

    @_on_stream
    def compress(self, centre: int = 0, *, max_bond_dim=np.inf, abs_err: float = 0, rel_err: float = 1e-12,
                 rank_tol: float = 1e-13) -> list[float]:
        """Globally optimal truncation of the finished register, in place: the sweep of :meth:`canonicalise`, cutting
        every bond's Schmidt values on the way back with the rule of the splits (``qsv_tensor_svd_split``): drop the
        longest tail whose sum stays ``<= max(abs_err, rel_err * sum)``, then cap at ``max_bond_dim``.  Returns the
        discarded weight per bond, ``sum(dropped s^2) / norm2()`` with ``norm2()`` taken before the sweep; the
        register ends in canonical form around ``centre``."""
        centre = self._check_centre(centre)
        if not (np.isfinite(rank_tol) and rank_tol >= 0):
            raise ValueError(f"rank_tol must be finite and >= 0, got {rank_tol}")
        if np.isnan(max_bond_dim) or max_bond_dim < 1:
            raise ValueError(f"max_bond_dim must be at least 1, got {max_bond_dim}")
        if not (abs_err >= 0 and rel_err >= 0):
            raise ValueError("abs_err and rel_err must be >= 0")
        m = len(self.sites)
        self._sweep_right(m - 1, rank_tol)
        kept = []

        def keep(s):
            kept.append(kept_rank(s, max_bond_dim, abs_err, rel_err))
            return kept[-1]

        met = self._sweep_left(0, rank_tol, keep)
        # the first bond met has isometries on its left and nothing cut yet: its Schmidt values square-sum to <psi|psi>,
        # which is norm2() before the sweep up to rounding, without the environment GEMMs norm2() would spend on it
        norm2 = float(np.sum(met[0] ** 2)) if met else 1.0
        weights = [float(np.sum(s[max(1, k):] ** 2) / norm2) for s, k in zip(met, kept)][::-1]
        self._sweep_right(centre, rank_tol)
        return weights

    @_on_stream
    def overlap(self, other: "SiteRegister") -> complex:
        """``sum conj(a) b`` over all amplitudes (``a`` = this register; no grid-measure factors) by the transfer-matrix
        recurrence of :meth:`_left_environment` with two chains: ``E' = sum_j A_j^H E B_j``, two GEMMs per site, the
        environment ``chi_a x chi_b``.  Neither register is contracted."""
        if not isinstance(other, SiteRegister):
            raise TypeError("overlap needs another SiteRegister")
        if len(other.sites) != len(self.sites) or other.d != self.d:
            raise ValueError("overlap needs registers with the same number of modes and the same grid size")
        if other.device != self.device:
            raise ValueError("overlap needs both registers on one device")
        torch = _torch()
        mine, theirs = self._torch_stream(), other._torch_stream()
        if theirs != mine:      # this stream reads the other register's sites: wait for what is queued on them
            ready = torch.cuda.Event()
            ready.record(theirs)
            mine.wait_event(ready)
        e = self._upload(np.ones((1, 1)))
        for a, b in zip(self.sites, other.sites):
            al, d, ar = (int(x) for x in a.shape)
            bl, _, br = (int(x) for x in b.shape)
            x = self._gemm(e, OP_NONE, b, OP_NONE, al, d * br, bl)                     # X[a, (j, b')]
            e = self._gemm(a, OP_CONJ_TRANSPOSE, x, OP_NONE, ar, br, al * d)          # E'[a', b']
        if theirs != mine:      # and the other stream must not overwrite or free those sites before the reads are done
            done = torch.cuda.Event()
            done.record(mine)
            theirs.wait_event(done)
        return complex(e.cpu().numpy()[0, 0])

    # ---- multi-shot sampling ----------------------------------------------------------------------------------
    @_on_stream
    def sample(self, uniforms: np.ndarray, operators=None, measure: float = 1.0):
        """``shots`` independent outcome lists of measuring every mode from the left (the chain ``Mq(0), Mq(0), ...`` of
        the reference, gates.py:87-117), all shots advancing together one site at a time on the device
        (``qsv_tensor_sample_site``); the register is not modified.

        ``uniforms``: ``(shots, m)`` numbers in [0, 1), ``uniforms[s, k]`` decides mode ``k`` of shot ``s`` the way
        ``rng.choice`` would with that draw.  ``operators[k]``: ``None`` or a ``(d, d)`` matrix applied to a copy of
        site ``k`` first (rotated quadratures).  ``measure``: the grid spacing ``dq``; the densities carry
        ``dq^(modes still unmeasured - 1)`` like ``MeasurementResult.probability``.  Returns ``picks (shots, m) int64``
        and ``densities (shots, m) float64``.

        The conditional weights need the right environment of every site (the registers here are not in canonical
        form): one right-to-left pass of the ``_right_environment`` recurrence whose intermediate ``site . E`` is kept
        per site and handed to the kernel next to the site itself."""
        torch = _torch()
        uniforms = np.asarray(uniforms, dtype=np.float64)
        m = len(self.sites)
        if uniforms.ndim != 2 or uniforms.shape[1] != m or uniforms.shape[0] < 1 or m < 1:
            raise ValueError(f"uniforms must have shape (shots >= 1, {m}), got {uniforms.shape}")
        if operators is not None and len(operators) != m:
            raise ValueError(f"operators must have one entry per mode ({m}), got {len(operators)}")
        shots = int(uniforms.shape[0])
        sites = list(self.sites)
        if operators is not None:
            for k, op in enumerate(operators):
                if op is None:
                    continue
                t = sites[k]
                cl, d, cr = (int(x) for x in t.shape)
                if np.shape(op) != (d, d):
                    raise ValueError(f"operators[{k}] must be a ({d}, {d}) matrix")
                out = self._empty(cl, d, cr)
                _lib.call("qsv_tensor_apply_axis_dev", self.device, self._stream(), self._p(t), self._p(out), cl, d, d, cr,
                          self._p(self._keep(op)))
                sites[k] = out
        # dressed[k] = (measured) site_k . E_k, E_k the environment of everything to the right of k (None at the right end:
        # E = 1).  The chain rotates a mode only when its turn comes, so E_k is built from the sites as they are -- a
        # rotation sampled on a finite grid is not exactly unitary, and the reference's densities show the difference.
        dressed = [None] * m
        r = None
        for k in range(m - 1, -1, -1):
            t = self.sites[k]
            cl, d, cr = (int(x) for x in t.shape)
            y = self._gemm(t, OP_NONE, r, OP_NONE, cl * d, cr, cr) if r is not None else None       # Y[(i, c), b]
            if r is not None:
                dressed[k] = y if sites[k] is t else self._gemm(sites[k], OP_NONE, r, OP_NONE, cl * d, cr, cr)
            if k > 0:
                r = self._gemm(y if y is not None else t, OP_NONE, t, OP_CONJ_TRANSPOSE, cl, cl, d * cr)
        u = self._upload(np.ascontiguousarray(uniforms.T), np.float64)          # (m, shots): one contiguous row per site
        picks = torch.empty((m, shots), dtype=torch.int32, device=self._dev)
        densities = torch.empty((m, shots), dtype=torch.float64, device=self._dev)
        v = self._upload(np.ones((shots, 1)))
        for k, t in enumerate(sites):
            cl, d, cr = (int(x) for x in t.shape)
            v_next = self._empty(shots, cr) if k + 1 < m else None
            _lib.call("qsv_tensor_sample_site", self.device, self._stream(), self._p(v), self._p(t),
                      self._p(dressed[k]) if dressed[k] is not None else None, shots, cl, d, cr,
                      float(measure) ** (m - 1 - k), self._p(u[k]), self._p(picks[k]), self._p(densities[k]),
                      self._p(v_next) if v_next is not None else None)
            v = v_next
        return (np.ascontiguousarray(picks.cpu().numpy().T.astype(np.int64)),
                np.ascontiguousarray(densities.cpu().numpy().T))

    # ---- gates ------------------------------------------------------------------------------------------------
    @_on_stream
    def apply_mode(self, operator: np.ndarray, mode: int) -> None:
        t = self.sites[mode]
        cl, d, cr = (int(x) for x in t.shape)
        op = self._keep(operator)
        if operator.ndim == 1:
            _lib.call("qsv_tensor_scale_axis", self.device, self._stream(), self._p(t), cl, d, cr, self._p(op))
            return
        out = self._empty(cl, int(operator.shape[0]), cr)
        _lib.call("qsv_tensor_apply_axis_dev", self.device, self._stream(), self._p(t), self._p(out), cl, d,
                  int(operator.shape[0]), cr, self._p(op))
        self.sites[mode] = out

    def _two_site(self, left: int):
        a, b = self.sites[left], self.sites[left + 1]
        cl, d, chi = (int(x) for x in a.shape)
        cr = int(b.shape[2])
        theta = self._gemm(a, OP_NONE, b, OP_NONE, cl * d, d * cr, chi, scratch="theta")
        return theta, cl, d, cr

    @_on_stream
    def _split(self, theta, rows: int, cols: int, *, max_bond_dim=np.inf, abs_err: float = 0, rel_err: float = 1e-12,
               rng_seed=None):
        """``tensor_svd`` (mps.py:52-97) of the device matrix ``theta``: exact SVD, or -- exactly when the reference does,
        ``max_bond_dim * 10 < min(rows, cols)`` -- the randomized range finder with the Gaussian test matrix drawn
        from ``rng_seed`` the way ``randomized_range_finder`` draws it (mps.py:14-15)."""
        full = min(rows, cols)
        capped = np.isfinite(max_bond_dim)
        cap = max(0, min(full, int(max_bond_dim))) if capped else full
        m1, m2 = self._scratch("m1", rows, max(cap, 1)), self._scratch("m2", max(cap, 1), cols)
        rank = C.c_uint64(0)
        if capped and max_bond_dim * 10 < full and cap >= 1:
            k = int(max_bond_dim)
            probes, power_iterations = k + 10, (7 if k < 0.1 * full else 4)
            s = np.empty(k, dtype=np.float64)
            # The first call goes without the Gaussian test matrix: under a loose tolerance the library's verified
            # low-rank route decides the split without reading it.  The reference draws it from default_rng(rng_seed)
            # (mps.py:14-15): a Generator handed down by the simulator (gates.py passes its own) is advanced by that draw,
            # so it is made in any case -- on a helper thread while the library works (both release the GIL) -- and only
            # the conversion and upload wait for the library to ask; a seed or None creates a generator nobody else sees,
            # and the draw itself waits too.
            draw = lambda: np.random.default_rng(rng_seed).normal(0, 1, size=(full, probes))
            if isinstance(rng_seed, np.random.Generator) and self._draw_pool is None:
                self._draw_pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix="qsv-omega")
            pending = self._draw_pool.submit(draw) if isinstance(rng_seed, np.random.Generator) else None
            dev_omega = None
            try:
                for attempt in range(2):
                    _lib.call("qsv_tensor_rsvd_split", self.device, self._stream(), self._p(theta), rows, cols, k, probes,
                              power_iterations, self._p(dev_omega) if dev_omega is not None else None, float(abs_err),
                              float(rel_err), self._p(m1), self._p(m2), cap, C.byref(rank), s.ctypes.data_as(C.c_void_p))
                    if rank.value != _lib.RANK_NEEDS_OMEGA:
                        break
                    omega = pending.result() if pending is not None else draw()
                    pending = None
                    dev_omega = self._upload(np.asfortranarray(omega).T)      # the transpose's C order = column-major omega
            finally:
                if pending is not None:
                    pending.result()          # the caller's generator must have moved on before anyone else draws
            self.split_counts["randomized"] += 1
        else:
            s = np.empty(full, dtype=np.float64)
            _lib.call("qsv_tensor_svd_split", self.device, self._stream(), self._p(theta), rows, cols,
                      int(max_bond_dim) if capped else -1, float(abs_err), float(rel_err), self._p(m1), self._p(m2),
                      cap, C.byref(rank), s.ctypes.data_as(C.c_void_p))
            self.split_counts["exact"] += 1
        r = int(rank.value)
        self.last_singular_values = s
        # the library wrote compact (rows x r) and (r x cols) matrices at the start of the buffers; copy them out so that
        # the sites do not pin buffers sized for the untruncated rank (theta-sized when there is no cap)
        return (m1.view(-1)[: rows * r].view(rows, r).clone(), m2.view(-1)[: r * cols].view(r, cols).clone(), r)

    def _store_pair(self, left: int, m1, m2, cl: int, cr: int, r: int) -> None:
        self.sites[left] = m1.reshape(cl, self.d, r)
        self.sites[left + 1] = m2.reshape(r, self.d, cr)

    @_on_stream
    def apply_two_mode(self, plane: np.ndarray, mode0: int, mode1: int, **truncation) -> None:
        """``theta[a, j, l, b] *= plane[j, l]`` (legs in the order ``mode0, mode1``), then split: CZ (gates.py:151-163)."""
        left = min(mode0, mode1)
        if mode0 > mode1:
            plane = np.ascontiguousarray(plane.T)
        theta, cl, d, cr = self._two_site(left)
        dev_plane = self._keep(plane)
        _lib.call("qsv_tensor_plane_diag", self.device, self._stream(), self._p(theta), cl, d, cr, self._p(dev_plane))
        m1, m2, r = self._split(theta, cl * d, d * cr, **truncation)
        self._store_pair(left, m1, m2, cl, cr, r)

    @_on_stream
    def apply_two_mode_gather(self, cols: np.ndarray, weights: np.ndarray, mode0: int, mode1: int, **truncation) -> None:
        """Resample every ``(q_left, q_right)`` plane of theta with the row-sparse table, then split: BS, CX
        (gates.py:58-84,166-192) and SWAP (gates.py:48-55; the table is the transposition)."""
        if mode0 > mode1:
            raise ValueError("plane tables are built for (left, right) order")
        left = mode0
        theta, cl, d, cr = self._two_site(left)
        per_point = int(cols.shape[-1]) if cols.ndim > 1 else 1
        dev_cols = self._keep(cols, np.int32)
        dev_vals = self._keep(weights, np.complex128)
        mapped = self._scratch("mapped", cl * d, d * cr)
        _lib.call("qsv_tensor_plane_gather", self.device, self._stream(), self._p(theta), self._p(mapped), cl, d, cr,
                  per_point, self._p(dev_cols), self._p(dev_vals))
        m1, m2, r = self._split(mapped, cl * d, d * cr, **truncation)
        self._store_pair(left, m1, m2, cl, cr, r)

    @_on_stream
    def apply_plane_phase(self, grid: np.ndarray, strength: float, left: int, **truncation) -> None:
        """CZ with the phases ``exp(i strength q_j q_l)`` evaluated in the kernel (no ``(d, d)`` table)."""
        theta, cl, d, cr = self._two_site(left)
        _lib.call("qsv_tensor_plane_phase", self.device, self._stream(), self._p(theta), cl, d, cr,
                  self._p(self._keep(grid, np.float64)), float(strength))
        m1, m2, r = self._split(theta, cl * d, d * cr, **truncation)
        self._store_pair(left, m1, m2, cl, cr, r)

    @_on_stream
    def apply_plane_affine(self, grid: np.ndarray, coefficients, left: int, **truncation) -> None:
        """BS / CX: resample every plane at ``(a00 x + a01 y, a10 x + a11 y)``, bilinear, computed in the kernel."""
        theta, cl, d, cr = self._two_site(left)
        mapped = self._scratch("mapped", cl * d, d * cr)
        a = (C.c_double * 4)(*[float(v) for v in coefficients])
        _lib.call("qsv_tensor_plane_affine", self.device, self._stream(), self._p(theta), self._p(mapped), cl, d, cr,
                  self._p(self._keep(grid, np.float64)), a)
        m1, m2, r = self._split(mapped, cl * d, d * cr, **truncation)
        self._store_pair(left, m1, m2, cl, cr, r)

    @_on_stream
    def project(self, mode: int, level: int, scale: float) -> None:
        """Keep grid point ``level`` of ``mode`` (times ``scale``) and absorb the bond matrix into a neighbour, on the
        side the reference picks (gates.py:108-115): into the left neighbour iff the slice is at least as tall as wide
        (``np.argmax(mode.shape) == 0``) and there is a left neighbour."""
        t = self.sites[mode]
        cl, d, cr = (int(x) for x in t.shape)
        bond = self._empty(cl, cr)
        _lib.call("qsv_tensor_take_level", self.device, self._stream(), self._p(t), self._p(bond), cl, d, cr, int(level),
                  float(scale))
        if cl >= cr and mode != 0:
            nb = self.sites[mode - 1]
            ncl, nd, _ = (int(x) for x in nb.shape)
            self.sites[mode - 1] = self._gemm(nb, OP_NONE, bond, OP_NONE, ncl * nd, cr, cl).reshape(ncl, nd, cr)
        else:
            nb = self.sites[mode + 1]
            _, nd, ncr = (int(x) for x in nb.shape)
            self.sites[mode + 1] = self._gemm(bond, OP_NONE, nb, OP_NONE, cl, nd * ncr, cr).reshape(cl, nd, ncr)
        self.sites.pop(mode)

    @_on_stream
    def insert(self, mode: int, vec: np.ndarray, **truncation) -> None:
        """New mode at ``mode``: a free-standing site at either end, otherwise attached to the site now at ``mode``
        and split off again (gates.py:24-45)."""
        n = len(self.sites)
        if mode == 0 or mode == n:
            self.sites.insert(mode, self._upload(np.asarray(vec).reshape(1, -1, 1)))
            return
        t = self.sites[mode]
        cl, d, cr = (int(x) for x in t.shape)
        dev_vec = self._upload(vec)
        joined = self._scratch("theta", cl * d, d * cr)          # [a, i, (j, b)] = vec[i] * t[a, (j, b)]
        _lib.call("qsv_tensor_insert_axis", self.device, self._stream(), self._p(t), self._p(joined), cl, d, d * cr,
                  self._p(dev_vec))
        m1, m2, r = self._split(joined, cl * d, d * cr, **truncation)
        self.sites[mode] = m2.reshape(r, d, cr)
        self.sites.insert(mode, m1.reshape(cl, d, r))

    # ---- GKP layer (gkp_simulator) ----------------------------------------------------------------------------
    def _outer(self, p, q, x: int, y: int, z: int, w: int, swap_last: bool):
        out = self._scratch("theta", x * y, z * w)
        _lib.call("qsv_tensor_outer", self.device, self._stream(), self._p(p), self._p(q), self._p(out), x, y, z, w,
                  int(swap_last))
        return out

    @_on_stream
    def insert_bond_pair(self, mode: int, first: np.ndarray, second: np.ndarray, **truncation) -> None:
        """Insert two new modes at ``mode`` that share a bond: ``first`` is ``(d, chi)``, ``second`` ``(chi, d)`` (a GKP
        Bell pair has chi = 2).  At the ends of the chain they are simply attached; inside, each half is multiplied into
        its neighbour and split off again (``InsertBell.apply``, gkp_simulator/insert_bell.py:60-96)."""
        d, chi = first.shape
        if mode == 0 or mode == len(self.sites):
            pair = [self._upload(first.reshape(1, d, chi)), self._upload(second.reshape(chi, d, 1))]
            self.sites[mode:mode] = pair
            return
        t1, t2 = self.sites[mode - 1], self.sites[mode]
        a, _, b = (int(v) for v in t1.shape)
        c = int(t2.shape[2])
        # [(a, i), k, b, dd] = t1[(a, i), b] * first[k, dd]  ->  rows (a, i), columns (k, b, dd)
        joined = self._outer(t1, self._keep(first), a * d, d, b, chi, swap_last=False)       # read only: a cached copy will do
        m1, m2, r1 = self._split(joined, a * d, d * b * chi, **truncation)
        new_t1, new_first = m1.reshape(a, d, r1), m2.reshape(r1, d, b * chi)
        # [b, dd, l, (j, c)] = second[dd, l] * t2[b, (j, c)]  ->  rows (b, dd, l), columns (j, c)
        joined = self._outer(t2, self._keep(second), b, chi, d * c, d, swap_last=True)
        m1, m2, r2 = self._split(joined, b * chi * d, d * c, **truncation)
        new_second, new_t2 = m1.reshape(b * chi, d, r2), m2.reshape(r2, d, c)
        self.sites[mode - 1:mode + 1] = [new_t1, new_first, new_second, new_t2]

    @_on_stream
    def operator_string_coefficients(self, operators: list[np.ndarray]) -> np.ndarray:
        """``C[i_0, ..., i_{m-1}] = <psi| O_{i_0} (x) ... (x) O_{i_{m-1}} |psi>`` (no grid-measure factors) for every
        string over the given single-mode operators: the contraction loop of ``full_logical_density_mps``
        (gkp_simulator/utils.py:82-90) as a depth-first walk that shares the environments of common prefixes."""
        n, k = len(self.sites), len(operators)
        dressed = []
        for t in self.sites:
            cl, d, cr = (int(v) for v in t.shape)
            row = []
            for op in operators:
                out = self._empty(cl, d, cr)
                _lib.call("qsv_tensor_apply_axis_dev", self.device, self._stream(), self._p(t), self._p(out), cl, d, d, cr,
                          self._p(self._keep(op)))
                row.append(out)
            dressed.append(row)
        result = np.zeros((k,) * n, dtype=np.complex128)

        def walk(level: int, g, prefix: tuple):
            if level == n:
                result[prefix] = np.conj(g.cpu().numpy()[0, 0])
                return
            bra = self.sites[level]
            cl, d, cr = (int(v) for v in bra.shape)
            for i in range(k):
                x = self._gemm(g, OP_CONJ_TRANSPOSE, dressed[level][i], OP_NONE, cl, d * cr, cl)
                walk(level + 1, self._gemm(x, OP_CONJ_TRANSPOSE, bra, OP_NONE, cr, cr, cl * d), prefix + (i,))

        walk(0, self._upload(np.ones((1, 1))), ())
        return result

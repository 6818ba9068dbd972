"""PSF reconstruction from the covariance of the ROKET error buffers: the Vii algorithm (reference: guardians/gamora.py,
psf_rec_Vii :24-100 and psf_rec_vii_cpu :103-171; the file it reads is what roket.VecRoket.save writes).

fft_size, telescope_otf   the size rule (:123) and the float64 host maps: otftel, den, mask (:124-133)
covmodes_from             P err err^T P^T / nframes of a sum of contributors (drax.get_err, get_err_contributors)
ViiReconstructor          covariance -> dphi, otf2, psf.  On a GPU the per-mode work runs on csrc/aomarl_psfrec.hip; on
                          the CPU the same statement runs in float64 NumPy -- that statement is the feature's definition.
psf_rec_vii               the reference's entry point: (otftel, otf2, psf) per environment, with the fitting OTF

With the eigenpairs (e_k, V_k) of the covariance and m_k = IF^T (Btt V_k)[:-2] + TT (Btt V_k)[-2:] on the lit pixels:
    tmp  = Re(fft2(sum_k e_k m_k^2) conj(fft2 pup)) - sum_k e_k |fft2 m_k|^2
    dphi = Re ifft2(2 tmp) . den . mask . (2 pi / lambda)^2,  otf2 = exp(-dphi / 2) . mask / max
    psf  = fftshift Re ifft2(otftel / max . otf2) . N^2 / npts
The reference transforms m_k^2 once per mode; the term is linear in m_k^2, so one transform of the weighted sum does."""
import ctypes as C

import numpy as np

from . import libaomarl as la
from . import roket

DEFAULT_SUM = ("noise", "aliasing", "tomography", "filtered modes", "non linearity", "bandwidth")   # drax.get_err's order


def fft_size(p):
    """gamora.py:123, evaluated as written: at a 2 p that is a power of two its value hangs on floating-point log."""
    mradix = 2
    return int(mradix ** int((np.log(2 * p) / np.log(mradix)) + 1))


def _binary_pupil(spup):
    spup = np.asarray(spup)
    if spup.ndim != 2 or spup.shape[0] != spup.shape[1]:
        raise ValueError("psf_rec: spup must be a square array, got shape %s" % (spup.shape,))
    if not np.all((spup == 0) | (spup == 1)):
        raise ValueError("psf_rec: spup is not binary (values other than 0 and 1): the Vii algorithm divides by the "
                         "pupil's autocorrelation and counts its lit pixels")
    return spup.astype(np.float64)


def telescope_otf(spup):
    """float64: dict(N, npts, pup [N][N], pupfft, otftel (normalised to its maximum), den, mask) (:123-133)."""
    spup = _binary_pupil(spup)
    p = spup.shape[0]
    N = fft_size(p)
    pup = np.zeros((N, N))
    pup[:p, :p] = spup
    pupfft = np.fft.fft2(pup)
    otftel = np.real(np.fft.ifft2(pupfft * np.conjugate(pupfft)))
    with np.errstate(divide="ignore"):
        den = 1.0 / otftel
    den[np.isinf(den)] = 0
    mask = np.ones((N, N))
    mask[otftel < 1e-5] = 0
    return dict(N=N, npts=int(np.count_nonzero(pup)), pup=pup, pupfft=pupfft, otftel=otftel / otftel.max(), den=den,
                mask=mask)


# ---------------------------------------------------------------------------------------------------- the file
def _as_dict(source):
    """VecRoket | path of an .npz | mapping -> a mapping with the keys VecRoket.save writes"""
    if isinstance(source, roket.VecRoket):
        if not source.keep_envs or not source.hist["x"]:
            raise ValueError("psf_rec: the source kept no histories (keep_envs=%r, %d frames): build the VecRoket with "
                             "keep_envs and run it" % (tuple(source.keep_envs), len(source.hist["x"])))
        return source.to_dict()
    if isinstance(source, (str, bytes)) or hasattr(source, "__fspath__"):
        with np.load(source) as z:
            return {k: z[k] for k in z.files}
    return source


def _env_index(d, env):
    envs = [int(e) for e in np.atleast_1d(d["envs"])] if "envs" in d else None
    if envs is None:
        return int(env)
    if int(env) not in envs:
        raise ValueError("psf_rec: environment %d is not among the kept ones, envs=%r" % (env, envs))
    return envs.index(int(env))


def _history(d, name, i):
    if name not in d:
        raise ValueError("psf_rec: the source has no kept histories: key %r is missing (a VecRoket needs keep_envs, a "
                         "file must come from VecRoket.save)" % name)
    h = np.asarray(d[name], dtype=np.float64)
    if h.ndim == 2:                                          # the reference's own layout: one environment
        return h
    if h.ndim != 3:
        raise ValueError("psf_rec: history %r has shape %s, not [envs][nactu][frames]" % (name, h.shape))
    return h[i]


def covmodes_from(source, env, contributors=None, rl=False):
    """P err err^T P^T / nframes for environment `env`.  contributors=None: the sum drax.get_err takes (plus zeta_com
    when rl); otherwise the named ones (drax.get_err_contributors / get_covmat_contrib)."""
    d = _as_dict(source)
    i = _env_index(d, env)
    names = list(DEFAULT_SUM) + (["zeta_com"] if rl else []) if contributors is None else list(contributors)
    if not names:
        raise ValueError("psf_rec: contributors is empty")
    err = sum(_history(d, n, i) for n in names)
    y = np.asarray(d["P"], dtype=np.float64).dot(err)
    return y.dot(y.T) / y.shape[1]


# ---------------------------------------------------------------------------------------------------- the product
class ViiReconstructor(object):
    """spup [p][p] binary; IF: the stack array's influence functions [nactu - 2][npts] (a SciPy sparse matrix or the
    file's (data, indices, indptr)); TT [npts][2]; Btt [nactu][nmodes]; tar_lambda in the unit of the phase (microns).
    device "cpu": float64 NumPy (dtype=np.float32: the same statement in single precision, what the GPU tests measure
    the arithmetic's own error with); a GPU device: csrc/aomarl_psfrec.hip."""

    def __init__(self, spup, IF, TT, Btt, tar_lambda, device="cpu", dtype=np.float64):
        import scipy.sparse as sp
        self.tel = t = telescope_otf(spup)
        self.N, self.npts, self.p = t["N"], t["npts"], np.asarray(spup).shape[0]
        if isinstance(IF, (tuple, list)):
            IF = sp.csr_matrix(tuple(np.asarray(a) for a in IF))
        self.IF = IF = sp.csr_matrix(IF)
        self.Btt = np.asarray(Btt, dtype=np.float64)
        self.TT = np.asarray(TT, dtype=np.float64)
        self.nactu = self.Btt.shape[0]
        if IF.shape[0] == self.npts and IF.shape[1] == self.nactu - 2 and self.npts != self.nactu - 2:
            raise ValueError("psf_rec: IF is [npts][nactu - 2]; the file stores [nactu - 2][npts]")
        if IF.shape != (self.nactu - 2, self.npts) or self.TT.shape != (self.npts, 2):
            raise ValueError("psf_rec: IF %s, TT %s do not fit %d actuators and the %d lit pixels of spup" %
                             (IF.shape, self.TT.shape, self.nactu, self.npts))
        self.scale2 = (2.0 * np.pi / float(tar_lambda)) ** 2
        self.denmask = t["den"] * t["mask"] * self.scale2
        self.lit = np.flatnonzero(np.asarray(spup).reshape(-1)).astype(np.int32)     # np.where(spup) order
        self.dtype = np.dtype(dtype)
        self.device = str(device)
        self.ptr = None
        if self.device != "cpu":
            self._create()

    # ------------------------------------------------------------------------------------------ shared front end
    def modes_of(self, covmodes):
        """(com [nk][nactu] = (Btt V)^T, w [nk] = the eigenvalues) in float64; eigh: the covariance is symmetric"""
        c = np.asarray(covmodes, dtype=np.float64)
        if c.ndim != 2 or c.shape[0] != c.shape[1] or c.shape[0] != self.Btt.shape[1]:
            raise ValueError("psf_rec: covmodes %s for %d modes" % (c.shape, self.Btt.shape[1]))
        e, V = np.linalg.eigh(0.5 * (c + c.T))
        return np.ascontiguousarray(self.Btt.dot(V).T), e

    def reconstruct(self, covmodes, otf_fit=None):
        """covmodes [nmodes][nmodes] or [B][nmodes][nmodes] -> dict(otftel, otf2, dphi, psf, strehl); otf_fit [N][N]
        replaces otftel in the last product (the fitting OTF)."""
        c = np.asarray(covmodes)
        if c.ndim == 3:
            outs = [self.reconstruct(ci, otf_fit) for ci in c]
            return {k: np.stack([o[k] for o in outs]) for k in outs[0]}
        com, w = self.modes_of(c)
        if self.device == "cpu":
            dphi, otf2, psf = self._statement(com, w, otf_fit)
        else:
            self.reset()
            self.accumulate(com, w)
            dphi, otf2, psf = (a.cpu().numpy() for a in self.finish(otf_fit))
        return dict(otftel=self.tel["otftel"], otf2=otf2, dphi=dphi, psf=psf, strehl=float(psf.max()))

    # ------------------------------------------------------------------------------------------ the CPU statement
    def maps_of(self, com):
        """m_k on the lit pixels, [nk][npts]"""
        com = np.asarray(com, dtype=np.float64)
        return np.asarray(self.IF.T.dot(com[:, :-2].T)).T + com[:, -2:].dot(self.TT.T)

    def _statement(self, com, w, otf_fit):
        f = self.dtype
        cplx = np.complex128 if f == np.float64 else np.complex64
        t, N, p = self.tel, self.N, self.p
        yy, xx = np.divmod(self.lit, p)
        w = np.asarray(w, dtype=f)
        m = self.maps_of(com).astype(f)
        var = np.zeros((N, N), dtype=f)
        acc = np.zeros((N, N), dtype=f)
        grid = np.zeros((N, N), dtype=f)
        for k in range(m.shape[0]):
            grid[yy, xx] = m[k]
            var[yy, xx] += w[k] * (m[k] * m[k])
            F = np.fft.fft2(grid).astype(cplx)
            acc += w[k] * (F.real * F.real + F.imag * F.imag)
        first = np.fft.fft2(var).astype(cplx) * np.conjugate(t["pupfft"]).astype(cplx)
        tmp = first.real - acc
        dphi = (np.fft.ifft2(2 * tmp).astype(cplx).real * self.denmask.astype(f)).astype(f)
        otf2 = np.exp(-0.5 * dphi) * t["mask"].astype(f)
        otf2 = otf2 / otf2.max()
        return dphi, otf2, self.psf_from(otf2, otf_fit)

    def psf_from(self, otf2, otf_fit=None):
        """the last product (:90-94) in the CPU statement's precision: fftshift Re ifft2(otf . otf2) . N^2 / npts"""
        f = self.dtype
        cplx = np.complex128 if f == np.float64 else np.complex64
        other = (self.tel["otftel"] if otf_fit is None else np.asarray(otf_fit)).astype(f)
        return np.fft.fftshift(np.fft.ifft2(other * np.asarray(otf2, dtype=f)).astype(cplx).real) * \
            f.type(self.N * self.N / float(self.npts))

    # ------------------------------------------------------------------------------------------ the native path
    def _create(self):
        import torch
        if not torch.cuda.is_available():
            raise la.AomarlError("ViiReconstructor(device=%r) needs a GPU; device=\"cpu\" is the float64 statement"
                                 % self.device)
        self.lib = la.load()
        self.tdev = torch.device(self.device)
        t = self.tel
        f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)                    # noqa: E731
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)                      # noqa: E731
        keep = [self.lit, f32(self.IF.data), i32(self.IF.indices), i32(self.IF.indptr), f32(self.TT), f32(self.denmask),
                f32(t["mask"]), f32(t["otftel"])]
        d = la.PsfRecDesc()
        d.p, d.N, d.npts, d.nactu, d.ld_actu = self.p, self.N, self.npts, self.nactu, self.nactu
        d.lit, d.if_data, d.if_indices, d.if_indptr = la.iptr(keep[0]), la.fptr(keep[1]), la.iptr(keep[2]), la.iptr(keep[3])
        d.tt, d.denmask, d.mask, d.otftel = (la.fptr(a) for a in keep[4:])
        ptr = C.c_void_p()
        with torch.cuda.device(self.tdev):
            la.check(self.lib.aomarl_psfrec_create(C.byref(d), C.byref(ptr)))
        self.ptr = ptr

    def __del__(self):
        if getattr(self, "ptr", None):
            self.lib.aomarl_psfrec_destroy(self.ptr)
            self.ptr = None

    def reset(self):
        la.check(self.lib.aomarl_psfrec_reset(self.ptr))

    def accumulate(self, com, w):
        """com [nk][nactu], w [nk] (host or device): acc and var take the vectors in index order"""
        import torch
        com = torch.as_tensor(np.asarray(com, dtype=np.float32) if not torch.is_tensor(com) else com,
                              dtype=torch.float32, device=self.tdev).contiguous()
        w = torch.as_tensor(np.asarray(w, dtype=np.float32) if not torch.is_tensor(w) else w, dtype=torch.float32,
                            device=self.tdev).contiguous()
        if com.dim() != 2 or com.shape[1] != self.nactu or w.shape != (com.shape[0],):
            raise ValueError("psf_rec: com %s, w %s for %d actuators" % (tuple(com.shape), tuple(w.shape), self.nactu))
        la.check(self.lib.aomarl_psfrec_accumulate(self.ptr, com.data_ptr(), w.data_ptr(), int(com.shape[0]),
                                                   la.raw_stream(self.tdev)))

    def finish(self, otf_fit=None):
        """(dphi, otf2, psf): device tensors [N][N]; the accumulated state stays as it is"""
        import torch
        out = [torch.empty(self.N, self.N, dtype=torch.float32, device=self.tdev) for _ in range(3)]
        fit = None
        if otf_fit is not None:
            fit = torch.as_tensor(np.ascontiguousarray(otf_fit, dtype=np.float32), device=self.tdev)
            if tuple(fit.shape) != (self.N, self.N):
                raise ValueError("psf_rec: otf_fit %s, N = %d" % (tuple(fit.shape), self.N))
        la.check(self.lib.aomarl_psfrec_finish(self.ptr, fit.data_ptr() if fit is not None else None, out[0].data_ptr(),
                                               out[1].data_ptr(), out[2].data_ptr(), la.raw_stream(self.tdev)))
        return tuple(out)


def fitting_otf(psfortho, N):
    """Re fft2(psfortho) / max (:85-89).  The reference's file holds psfortho with the zero frequency at [0, 0]
    (roket_generalized_rl.py:424 undoes get_tar_image's shift); VecRoket.save writes the mean of target_image's frames
    as they come, zero frequency at [N/2, N/2], so the shift is undone here."""
    psfortho = np.asarray(psfortho, dtype=np.float64)
    if psfortho.shape != (N, N):
        raise ValueError("psf_rec: psfortho is %s but N = %d: the fitting PSF must be sampled on the reconstruction's "
                         "grid" % (psfortho.shape, N))
    otf = np.real(np.fft.fft2(np.fft.ifftshift(psfortho)))
    return otf / otf.max()


def from_source(source, device=None, dtype=np.float64):
    """(dict of the file's keys, ViiReconstructor) of a VecRoket, an .npz path or a mapping"""
    d = _as_dict(source)
    for k in ("spup", "tar_lambda"):
        if k not in d:
            raise ValueError("psf_rec: the source lacks %r (files written before the reconstruction existed do)" % k)
    if device is None:
        device = str(source.device) if isinstance(source, roket.VecRoket) else "cpu"
    rec = ViiReconstructor(d["spup"], (d["IF.data"], d["IF.indices"], d["IF.indptr"]), d["TT"], d["Btt"],
                           float(np.asarray(d["tar_lambda"]).reshape(-1)[0]), device=device, dtype=dtype)
    return d, rec


def psf_rec_vii(source, envs=None, err=None, fitting=True, covmodes=None, cov=None, rl=False, device=None, rec=None):
    """gamora.psf_rec_Vii (:24-100): (otftel, otf2, psf) of every environment of `envs` (default: all the kept ones; an
    int: that environment alone, one tuple).  err [nactu][frames]: error buffers instead of the file's sum; covmodes:
    their covariance in actuator space (projected with P, :60); cov: the covariance in modal space, as it is (:63)."""
    if rec is None:
        d, rec = from_source(source, device)
    else:
        d = _as_dict(source)
    single = envs is not None and np.ndim(envs) == 0
    kept = [int(e) for e in np.atleast_1d(d["envs"])] if "envs" in d else [0]
    todo = kept if envs is None else [int(e) for e in np.atleast_1d(envs)]
    P = np.asarray(d["P"], dtype=np.float64)
    out = []
    for e in todo:
        if cov is not None:
            cm = np.asarray(cov, dtype=np.float64)
        elif covmodes is not None:
            cm = P.dot(np.asarray(covmodes, dtype=np.float64)).dot(P.T)
        elif err is not None:
            y = P.dot(np.asarray(err, dtype=np.float64))
            cm = y.dot(y.T) / y.shape[1]
        else:
            cm = covmodes_from(d, e, rl=rl)
        fit = None
        if fitting and "psfortho" in d:
            po = np.asarray(d["psfortho"])
            if po.ndim == 3:
                who = [int(x) for x in np.atleast_1d(d["psfortho_envs"])] if "psfortho_envs" in d else kept
                if e not in who:
                    raise ValueError("psf_rec: psfortho was kept for environments %r, not for %d" % (who, e))
                po = po[who.index(e)]
            fit = fitting_otf(po, rec.N)
        r = rec.reconstruct(cm, fit)
        out.append((r["otftel"], r["otf2"], r["psf"]))
    return out[0] if single else out

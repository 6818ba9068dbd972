"""What the sensors that attach to a VecRlSupervisor's loop share (pyramid.PyramidSensor, lgs.LgsSensor): the commands
through the mirrors in chunks of `nenv` (registration.DmRegistration.calibrate drives its pushes through the same
function), the calibration on the Btt modes, start / stop, the frame of next_part_one and the integrator on the
sensor's own command matrix."""
import numpy as np

from . import attachments

__all__ = ["LoopSensor", "padded_volts", "through_mirrors", "host_rows"]


def padded_volts(sim, volts):
    """volts [n <= nenv][nactu] as the float32 commands of all `nenv` environments (the rest zero), where the simulator
    takes them: a device tensor, or the array itself for a CPU simulator"""
    v = np.zeros((sim.nenv, volts.shape[1]), dtype=np.float32)
    v[:volts.shape[0]] = volts
    if str(sim.device) == "cpu":
        return v
    import torch
    return torch.from_numpy(v).to(sim.device)


def host_rows(t, nn):
    """the first nn rows of a simulator's array or tensor as float64 on the host (a copy: the buffer is written again)"""
    return np.array(t[:nn], dtype=np.float64) if isinstance(t, np.ndarray) else t[:nn].double().cpu().numpy()


def through_mirrors(sim, volts, read):
    """The commands volts [K][nactu] through the simulator's mirrors (comp_dm_shape), nenv at a time; read(nn) gives what
    the nn commands of the chunk just shaped leave, [nn][...] on the host.  Returns the K rows."""
    rows = []
    for k0 in range(0, volts.shape[0], sim.nenv):
        chunk = volts[k0:k0 + sim.nenv]
        sim.comp_dm_shape(padded_volts(sim, chunk))
        rows.append(read(chunk.shape[0]))
    return np.concatenate(rows)


class LoopSensor(object):
    """A subclass supplies `slot` (its row of attachments.TABLE), `sup`, `native` (image, slopes, set_ref), `nslope`,
    `device`, `_pupil()` (the mask of its pupil in the simulator's sensor phase buffer), `_quiet()` (its noise-free
    measure of that buffer), `_trace()` and `_measure()` (the loop's frame), and sets `cmat`, `ref`, `linearity`,
    `_cmat_dev` to None and `_attached` to False."""
    slot = None
    # the frame's phase copy (keep_wfs_phase) is taken from the buffer the sensor just measured; False: the
    # supervisor traces it once more behind the frame (_snap_wfs_phase)
    keeps_phase = False

    row = property(lambda self: attachments.TABLE[self.slot])

    # ---- measurements
    @property
    def image(self):
        return self.native.image

    @property
    def slopes(self):
        return self.native.slopes

    def set_ref(self, ref=None):
        self.native.set_ref(ref)
        self.ref = None if ref is None else np.asarray(ref, dtype=np.float32).copy()

    # ---- calibration
    def _volts(self, volts):
        return padded_volts(self.sup.sim, volts)

    def _mirrors_only(self, volts, read):
        sim = self.sup.sim

        def traced(nn):
            sim.raytrace_wfs(atm=False, dms=True, reset=True)
            return read(nn)
        return through_mirrors(sim, volts, traced)

    def _response(self, volts):
        """Noise-free slopes [K][nslope] (float64, host) of the commands volts [K][nactu], atmosphere off."""
        def read(nn):
            self._quiet()
            return host_rows(self.native.slopes, nn)
        return self._mirrors_only(volts, read)

    def _phase_rms(self, volts):
        """The rms of the sensor's pupil phase [K] (float64, host) of the commands volts [K][nactu], atmosphere off."""
        sim, pup = self.sup.sim, self._pupil()

        def read(nn):
            ph = host_rows(sim.t["wfs_phase"].reshape(sim.nenv, -1), nn)[:, pup]
            return np.sqrt(((ph - ph.mean(axis=1, keepdims=True))**2).mean(axis=1))
        return self._mirrors_only(volts, read)

    def calibrate(self, push_um=0.01):
        """Flat reference slopes, the Btt modes pushed and pulled through the mirrors by `push_um` microns rms of phase
        each, the same with twice the push -- `self.linearity` is the largest relative deviation of a mode's response
        per unit push between the two -- and the command matrix through modal.cmat_with_btt with the supervisor's
        filtered-mode count.  Leaves the mirrors of the simulator as the supervisor's voltages say.  Returns the
        command matrix [nactu][nslope]."""
        from . import modal
        sup = self.sup
        if sup is None:
            raise RuntimeError("calibrate: a stand-alone sensor has no mirrors")
        if self._attached:
            raise RuntimeError("calibrate: stop() first")
        m2v = np.asarray(sup.modes2volts, dtype=np.float64)             # [nactu][nmodes]
        v2m = np.asarray(sup.volts2modes, dtype=np.float64)             # [nmodes][nactu]
        self.native.set_ref(None)
        flat = self._response(np.zeros((1, m2v.shape[0])))[0]
        self.set_ref(flat)
        # rms of the sensor's pupil phase per unit of each mode: the Btt modes are orthonormal for the geometric
        # covariance (modal.compute_btt), measured here rather than assumed
        a = push_um / np.maximum(self._phase_rms(m2v.T), 1e-30)
        cmds = m2v.T * a[:, None]
        d1 = (self._response(cmds) - self._response(-cmds)) / (2 * a[:, None])
        d2 = (self._response(2 * cmds) - self._response(-2 * cmds)) / (4 * a[:, None])
        n1 = np.linalg.norm(d1, axis=1)
        self.linearity = float(np.max(np.linalg.norm(d2 - d1, axis=1) / np.maximum(n1, 1e-300)))
        self.push = a
        self.imat_modes = d1.T                                          # [nslope][nmodes]
        nfilt = max(int(getattr(sup, "n_reverse_filtered_from_cmat", 0)), 0)
        self.cmat = modal.cmat_with_btt(self.imat_modes @ v2m, m2v, nfilt)
        self._cmat_dev = None
        sim = sup.sim                                                   # the mirrors back on the loop's voltages
        if str(sim.device) == "cpu":
            sim.comp_dm_shape(np.asarray(sim.voltage)[:, :m2v.shape[0]])
        else:
            sim.comp_dm_shape()
        return self.cmat

    # ---- the loop
    def start(self):
        """Attach: the supervisor's next_part_one measures with this sensor (see VecRlSupervisor.next_part_one)."""
        sup, who = self.sup, self.row.who
        if sup is None:
            raise RuntimeError(who + ": a stand-alone sensor has no loop")
        if self.cmat is None:
            raise RuntimeError(who + ": calibrate() first")
        attachments.attach(sup, self.slot, self)
        if str(sup.sim.device) != "cpu" and self._cmat_dev is None:
            import torch
            self._cmat_dev = torch.as_tensor(np.ascontiguousarray(self.cmat, dtype=np.float32), device=sup.sim.device)
        self._attached = True
        return self

    def stop(self):
        if self._attached:
            attachments.detach(self.sup, self.slot, self)
            self._attached = False

    def frame(self, move_atmos):
        """The frame of next_part_one behind the move: target PSF, the sensor's pupil phase, the next move's prefetch,
        image and slopes.  Returns whether it kept the frame's phase copy."""
        sup, sim = self.sup, self.sup.sim
        sim.target_psf()
        self._trace()
        if sup.prefetch_atmos and move_atmos:
            sim.prefetch_atmos()
        self._measure()
        if self.keeps_phase and sup.keep_wfs_phase:
            sup._keep_wfs_phase_buffer()
            return True
        return False

    def control(self):
        """err = -cmat . slopes into the state's err, com += gain err (the supervisor's next_part_one calls it)."""
        sup, sim = self.sup, self.sup.sim
        sim.gemm_nt(self.native.slopes, self._cmat_dev, alpha=-1.0, beta=0.0, Cout=sim.err)
        sim.com.add_(sim.err, alpha=float(sup.gain))

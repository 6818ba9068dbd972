"""Loop attachments: the objects that hang on a VecRlSupervisor between their start() and stop().

One table (TABLE), one row per attachment: the slot on the supervisor, the words of the messages, what the attachment
does to the loop (the flags) and the supervisor conditions it refuses.  Which attachments exclude each other follows
from the flags (`excludes`), so it is the same in both orders of starting them:
  senses        it replaces the frame's sensing (its frame() in next_part_one): the environment runs the call-by-call
                path.  At most one.
  own_control   err comes from the sensor's own command matrix (its control()): no modal shortcut, no deferred control,
                get_slopes returns the sensor's slopes.  A registration senses without it: it calls the supervisor's
                do_control, with the supervisor's command matrix, which also feeds a control law.
  control_law   it lives inside do_control, which an own-control sensor never calls: the two exclude each other.
                Restarted by reset().  At most one.
  every_frame   (a control law) every frame has to reach do_control: no deferred control.
  reads_planes  it traces the mirror planes: next_part_two must not leave their shapes to the frame kernel.

attach() also keeps the supervisor's two plain attributes `sensing` and `control_law` (the attached object with that
flag, or None): what the per-step code of env.py reads.  DESIGN.md ("Loop attachments") has the derived matrix.
"""

__all__ = ["TABLE", "CONDITIONS", "excludes", "OPEN_LOOP", "refuse", "check", "attach", "detach", "le_strehl"]


def _sim(sup, name, default=None):
    return getattr(getattr(sup, "sim", None), name, default)


# name: (predicate on a supervisor -- an attribute it lacks counts as unset --, exception, message core)
CONDITIONS = {
    "frame_pipeline": (lambda sup: _sim(sup, "_twin") is not None, RuntimeError,
                       "the frame pipeline is on (build the environment with frame_pipeline=False)"),
    "reset_prefetch": (lambda sup: getattr(sup, "reset_prefetch", None) is not None, RuntimeError,
                       "a prefetched reset is set (reset_prefetch): not covered"),
    "pure_delay_0": (lambda sup: bool(getattr(sup, "pure_delay_0", False)), NotImplementedError,
                     "modification_online (the pure-delay-0 call order) is not covered"),
    "autoencoder": (lambda sup: getattr(sup, "autoencoder", None) is not None, RuntimeError,
                    "a denoiser (autoencoder) is set"),
    "geo": (lambda sup: getattr(sup, "geo", None) is not None, RuntimeError, "the GEO twin (geo=True) is not covered"),
    "modal_gains": (lambda sup: getattr(sup, "modal_gains", None) is not None, RuntimeError,
                    "modal gains are set (set_modal_gains(None) first)"),
    "env_gains": (lambda sup: getattr(sup, "gain", 0.0) is None or bool(getattr(sup, "_env_gains", False)), RuntimeError,
                  "the supervisor has per-environment gains (set_gain with a vector, set_env_gains); set one scalar "
                  "gain first"),
    "keep_image": (lambda sup: bool(getattr(sup, "keep_tar_image", False) or getattr(sup, "keep_le_image", False)),
                   RuntimeError, "keep_tar_image / keep_le_image: the full-frame target image traces for itself"),
    "screens_ahead": (lambda sup: bool(getattr(sup, "prefetch_atmos", False) or _sim(sup, "prefetch", False) or
                                       _sim(sup, "pending_atmos", False)), RuntimeError,
                      "the screens run one frame ahead (prefetch_atmos); build the environment with prefetch_atmos=False"),
}


class Row(object):
    """One attachment.  conditions: names of CONDITIONS, or (name, the row's own reason[, its exception class])."""

    def __init__(self, slot, cls, a, own, conditions, senses=False, own_control=False, control_law=False,
                 every_frame=False, reads_planes=False, materialize=False):
        self.slot, self.cls, self.who, self.a, self.own = slot, cls, cls + ".start", a, own
        self.conditions = conditions
        self.senses, self.own_control, self.control_law = senses, own_control, control_law
        self.every_frame, self.reads_planes, self.materialize = every_frame, reads_planes, materialize
        self.role = "sensing" if senses else "control_law"


_AHEAD = "the frames run a step ahead of the chains"
# what refuses a recording of the open loop (modal_gains.record_open_loop) and with it the two control laws
OPEN_LOOP = ("reset_prefetch", ("frame_pipeline", "slopes of odd frames live in its twin"), "pure_delay_0",
             ("autoencoder", "the loop model has no denoiser", NotImplementedError))

TABLE = {r.slot: r for r in (
    Row("pyramid", "PyramidSensor", "a pyramid", "a pyramid", senses=True, own_control=True, materialize=True,
        conditions=(("frame_pipeline", _AHEAD), "reset_prefetch", "pure_delay_0",
                    ("autoencoder", "the denoiser works on Shack-Hartmann spots, not on a pyramid"), "geo",
                    ("modal_gains", "the pyramid's loop is the scalar integrator"), "env_gains")),
    Row("lgs", "LgsSensor", "a laser guide star", "an LGS", senses=True, own_control=True, materialize=True,
        conditions=(("frame_pipeline", _AHEAD), "reset_prefetch", "pure_delay_0",
                    ("autoencoder", "the denoiser is trained on NGS spots and reads the simulator's cube, not the LGS "
                                    "sensor's"), "geo",
                    ("modal_gains", "the LGS loop is the scalar integrator"), "env_gains")),
    Row("registration", "DmRegistration", "a mirror mis-registration", "a registration", senses=True, reads_planes=True,
        materialize=True,
        conditions=(("frame_pipeline", "its frame kernel samples registered mirrors"), "reset_prefetch", "pure_delay_0",
                    ("geo", "it traces registered mirrors of its own"), ("autoencoder", "that path is not covered"),
                    ("keep_image", "through registered mirrors"))),
    Row("online_modal_gains", "OnlineModalGains", "an on-line modal-gain optimiser", "an on-line optimiser",
        control_law=True, conditions=OPEN_LOOP + ("env_gains",)),
    Row("modal_predictor", "ModalPredictor", "a modal predictor", "a predictor", control_law=True, every_frame=True,
        conditions=OPEN_LOOP + ("env_gains",)),
)}


def excludes(a, b):
    """Whether the attachments of slots a and b cannot be attached together (symmetric)."""
    ra, rb = TABLE[a], TABLE[b]
    return a == b or (ra.senses and rb.senses) or (ra.control_law and rb.control_law) or \
        (ra.own_control and rb.control_law) or (ra.control_law and rb.own_control)


def refuse(sup, who, conditions=(), slots=()):
    """Raise, in the name of `who`, for the first of `slots` that holds an attachment, then for the first of
    `conditions` that holds.  `sup.sim` is not read before the slots have passed."""
    for slot in slots:
        if getattr(sup, slot, None) is not None:
            raise RuntimeError("%s: %s is attached (%s.stop first)" % (who, TABLE[slot].a, TABLE[slot].cls))
    for c in conditions:
        name, reason, exc = (c, None, None) if isinstance(c, str) else (tuple(c) + (None,))[:3]
        holds, default, core = CONDITIONS[name]
        if holds(sup):
            raise (exc or default)("%s: %s%s" % (who, core, ": " + reason if reason else ""))


def check(sup, slot):
    """What attach refuses, without attaching."""
    row = TABLE[slot]
    if getattr(sup, slot, None) is not None:
        raise RuntimeError("%s: the supervisor has %s attached already" % (row.who, row.own))
    refuse(sup, row.who, row.conditions, [s for s in TABLE if s != slot and excludes(slot, s)])


def attach(sup, slot, obj):
    check(sup, slot)
    row = TABLE[slot]
    if row.materialize:
        sup.materialize_control()               # a frame still waiting for its do_control gets the law it was imaged under
    setattr(sup, slot, obj)
    setattr(sup, row.role, obj)


def detach(sup, slot, obj):
    """Clears the slot if it still holds `obj`; a second call is nothing."""
    if getattr(sup, slot, None) is obj:
        setattr(sup, slot, None)
        setattr(sup, TABLE[slot].role, None)


def le_strehl(sup, nframes):
    """long-exposure Strehl (mean over the environments) of `nframes` integrator frames behind a reset"""
    sup.reset()
    sup.next_part_one()
    for _ in range(nframes):
        sup.next_part_two(None, linear_control=True)
        sup.next_part_one()
    return float(sup.get_strehl()[:, 1].mean())

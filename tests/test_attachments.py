"""ao_marl_amd/attachments.py on SimpleNamespace supervisors: the exclusion matrix cell by cell, every (attachment,
condition) refusal of the table and every pair outside it, detach, a bare supervisor, and ROKET's refusal of a sensor."""
from types import SimpleNamespace as NS

import pytest

from ao_marl_amd import attachments as A

SLOTS = ["pyramid", "lgs", "registration", "online_modal_gains", "modal_predictor"]
# EXCLUDED[i][j]: SLOTS[i] refuses to start while SLOTS[j] is attached.  The matrix of the five start() methods as they
# stood one by one, plus the four cells (*) that were accepted and silently wrong: a control law started beside a
# sensor with its own control, whose frames never reach do_control.
EXCLUDED = [
    # pyr  lgs  reg  omg  pred
    [1,   1,   1,   1,   1],        # pyramid
    [1,   1,   1,   1,   1],        # lgs
    [1,   1,   1,   0,   0],        # registration: it runs the supervisor's do_control, which feeds a control law
    [1,   1,   0,   1,   1],        # online_modal_gains   (*) pyramid, lgs
    [1,   1,   0,   1,   1],        # modal_predictor      (*) pyramid, lgs
]

# condition -> the attributes that make it hold on a supervisor that otherwise lacks them
HOLDS = {
    "frame_pipeline": dict(sim=NS(_twin=object())),
    "reset_prefetch": dict(reset_prefetch="same"),
    "pure_delay_0": dict(pure_delay_0=True),
    "autoencoder": dict(autoencoder=object()),
    "geo": dict(geo=object()),
    "modal_gains": dict(modal_gains=[[1.0]]),
    "env_gains": dict(gain=None),
    "keep_image": dict(keep_le_image=True),
    "screens_ahead": dict(sim=NS(pending_atmos=True)),
}
# (attachment, condition) -> the exception: the table of DESIGN.md ("Loop attachments"), written out
R, N = RuntimeError, NotImplementedError
REFUSED = {
    "pyramid": dict(frame_pipeline=R, reset_prefetch=R, pure_delay_0=N, autoencoder=R, geo=R, modal_gains=R, env_gains=R),
    "lgs": dict(frame_pipeline=R, reset_prefetch=R, pure_delay_0=N, autoencoder=R, geo=R, modal_gains=R, env_gains=R),
    "registration": dict(frame_pipeline=R, reset_prefetch=R, pure_delay_0=N, autoencoder=R, geo=R, keep_image=R),
    "online_modal_gains": dict(frame_pipeline=R, reset_prefetch=R, pure_delay_0=N, autoencoder=N, env_gains=R),
    "modal_predictor": dict(frame_pipeline=R, reset_prefetch=R, pure_delay_0=N, autoencoder=N, env_gains=R),
}


def _sup(**kw):
    """a supervisor that lacks every optional attribute but what kw gives it"""
    return NS(materialize_control=lambda: None, **kw)


def test_the_table_is_the_one_written_out_here():
    assert list(A.TABLE) == SLOTS and set(A.CONDITIONS) == set(HOLDS)
    for slot, row in A.TABLE.items():
        names = [c if isinstance(c, str) else c[0] for c in row.conditions]
        assert sorted(names) == sorted(REFUSED[slot]) and row.slot == slot and row.who == row.cls + ".start"
    flags = {s: (r.senses, r.own_control, r.control_law, r.every_frame, r.reads_planes) for s, r in A.TABLE.items()}
    assert flags == dict(pyramid=(True, True, False, False, False), lgs=(True, True, False, False, False),
                         registration=(True, False, False, False, True),
                         online_modal_gains=(False, False, True, False, False),
                         modal_predictor=(False, False, True, True, False))


@pytest.mark.parametrize("i", range(5))
@pytest.mark.parametrize("j", range(5))
def test_exclusion_matrix(i, j):
    mine, other = SLOTS[i], SLOTS[j]
    assert EXCLUDED[i][j] == EXCLUDED[j][i] == int(A.excludes(mine, other)) == int(A.excludes(other, mine))
    there, obj = object(), object()
    sup = _sup(**{other: there})
    if EXCLUDED[i][j]:
        with pytest.raises(RuntimeError, match="attached") as info:
            A.attach(sup, mine, obj)
        assert A.TABLE[mine].who in str(info.value)
        assert (A.TABLE[other].own if i == j else A.TABLE[other].cls + ".stop first") in str(info.value)
        assert getattr(sup, other) is there and getattr(sup, mine, None) is (there if i == j else None)
    else:
        A.attach(sup, mine, obj)
        assert getattr(sup, mine) is obj and getattr(sup, other) is there


@pytest.mark.parametrize("slot", SLOTS)
@pytest.mark.parametrize("cond", sorted(HOLDS))
def test_every_condition_against_every_attachment(slot, cond):
    sup, obj = _sup(**HOLDS[cond]), object()
    assert A.CONDITIONS[cond][0](sup) and not A.CONDITIONS[cond][0](_sup())
    exc = REFUSED[slot].get(cond)
    if exc is None:
        A.attach(sup, slot, obj)
        assert getattr(sup, slot) is obj
        return
    with pytest.raises((RuntimeError, NotImplementedError)) as info:
        A.attach(sup, slot, obj)
    assert type(info.value) is exc and str(info.value).startswith(A.TABLE[slot].who + ": ")
    assert A.CONDITIONS[cond][2] in str(info.value)
    assert getattr(sup, slot, None) is None and getattr(sup, A.TABLE[slot].role, None) is None


def test_conditions_hold_on_either_of_their_attributes():
    for kw in (dict(keep_tar_image=True), dict(_env_gains=True), dict(prefetch_atmos=True), dict(sim=NS(prefetch=True))):
        name = [n for n, (holds, _, _) in A.CONDITIONS.items() if holds(_sup(**kw))]
        assert name in (["keep_image"], ["env_gains"], ["screens_ahead"]), kw
    with pytest.raises(RuntimeError, match="VecRoket: .*prefetch_atmos"):
        A.refuse(_sup(prefetch_atmos=True), "VecRoket", ("screens_ahead",))
    with pytest.raises(NotImplementedError, match="somebody: .*denoiser.*: no reason"):
        A.refuse(_sup(autoencoder=1), "somebody", (("autoencoder", "no reason", NotImplementedError),))


@pytest.mark.parametrize("slot", SLOTS)
def test_attach_and_detach_on_a_bare_supervisor(slot):
    calls = []
    sup = NS(materialize_control=lambda: calls.append(1))
    row, obj, other = A.TABLE[slot], object(), object()
    A.attach(sup, slot, obj)
    assert getattr(sup, slot) is obj and getattr(sup, row.role) is obj and len(calls) == int(row.materialize)
    assert row.role == ("sensing" if row.senses else "control_law")
    A.detach(sup, slot, other)                  # not the holder: nothing
    assert getattr(sup, slot) is obj and getattr(sup, row.role) is obj
    A.detach(sup, slot, obj)
    A.detach(sup, slot, obj)                    # a second time: nothing
    assert getattr(sup, slot) is None and getattr(sup, row.role) is None
    setattr(sup, slot, other)
    A.detach(sup, slot, obj)                    # a slot that holds another object stays
    assert getattr(sup, slot) is other
    A.detach(NS(), slot, obj)                   # a supervisor without the slot


def test_slots_are_declared_on_the_supervisor():
    from ao_marl_amd.env import VecRlSupervisor
    for name in SLOTS + ["sensing", "control_law"]:
        assert name in vars(VecRlSupervisor) and getattr(VecRlSupervisor, name) is None


def test_the_classes_name_their_rows():
    from ao_marl_amd.lgs import LgsSensor
    from ao_marl_amd.modal_gains import OnlineModalGains
    from ao_marl_amd.predictive import ModalPredictor
    from ao_marl_amd.pyramid import PyramidSensor
    from ao_marl_amd.registration import DmRegistration
    for cls in (PyramidSensor, LgsSensor, DmRegistration, OnlineModalGains, ModalPredictor):
        row = A.TABLE[cls.slot]
        assert row.cls == cls.__name__ and cls.__new__(cls).row is row
        assert all(hasattr(cls, m) for m in (("frame", "control") if row.senses else ("restart",)))


def test_control_laws_refuse_a_sensor_with_its_own_control():
    """the cells (*) through the start() methods themselves, before they touch the supervisor's modal gains"""
    from ao_marl_amd.modal_gains import OnlineModalGains
    from ao_marl_amd.predictive import ModalPredictor
    for cls in (OnlineModalGains, ModalPredictor):
        for slot, word in (("pyramid", "a pyramid is attached"), ("lgs", "a laser guide star is attached")):
            sup = NS(sim=NS(nenv=2), s=NS(delay=1.0), gain=0.4, nmodes=3, **{slot: object()})
            with pytest.raises(RuntimeError, match=word) as info:
                cls(sup).start()
            assert cls.__name__ + ".start" in str(info.value) and getattr(sup, cls.slot, None) is None


def test_roket_refuses_every_sensing_attachment_by_name():
    from ao_marl_amd import params, roket
    for slot, word in (("pyramid", "a pyramid is attached"), ("lgs", "a laser guide star is attached"),
                       ("registration", "a mirror mis-registration is attached")):
        sup = NS(sim=NS(), gain=0.7, geo=object(), config=params.builtin("production_sh_10x10_2m"), **{slot: object()})
        env = NS(supervisor=sup, frame_pipeline=False, rl_step=None)
        with pytest.raises(RuntimeError, match="VecRoket: " + word):
            roket._roket_supervisor(env)
        setattr(sup, slot, None)
        assert roket._roket_supervisor(env) is sup

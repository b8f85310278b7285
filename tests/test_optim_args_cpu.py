"""CPU (no GPU): what the eighteen optimiser-step entry points (``ce_{adam,sgd,lion}_step[_tiles|_groups][_ema]``) refuse whatever
their rule -- the checks of csrc/optim.hip's one host launcher, ``run_step``: the form (``n > 0``, or a table with something in it),
the buffers (``p``, ``g``, every state stream of the rule, ``p_bf16`` in the table forms), the group count, and the weight average
of the ``_ema`` twins.  One argument is made invalid at a time, on fake non-NULL pointers: validation precedes any launch, so
nothing here touches a device.  The rules' own scalar checks are in tests/test_sgd_cpu.py, test_lion_cpu.py, test_partial_cpu.py."""
from ctypes import c_float, c_int, c_long, c_void_p

import pytest

EINVAL = -22
FAKE = c_void_p(0x1000)           # a non-NULL pointer: a call that passed validation would launch on it (and fail: no device)
NULL = c_void_p(0)
FORMS = {"flat": "", "tiles": "_tiles", "groups": "_groups"}

# per rule: its state streams, and the scalars behind (sumsq, max_norm) -- in the grouped forms behind (groups, ngroups)
RULES = {
    "adam": dict(state=("m", "v"), null_state=b"null buffer",
                 plain=(c_float(0.1), c_float(0.9), c_float(0.999), c_float(1e-8), c_float(0.0), c_int(1)),
                 grouped=(c_float(0.9), c_float(0.999), c_float(1e-8), c_int(1))),
    "sgd": dict(state=("buf",), null_state=b"momentum buffer",                     # momentum 0.9: the buffer is needed
                plain=(c_float(0.1), c_float(0.9), c_float(0.0), c_float(0.0), c_int(0), c_int(1)),
                grouped=(c_float(0.9), c_float(0.0), c_int(0), c_int(1))),
    "lion": dict(state=("m",), null_state=b"momentum buffer",
                 plain=(c_float(0.1), c_float(0.9), c_float(0.99), c_float(0.0)),
                 grouped=(c_float(0.9), c_float(0.99))),
}
ENTRY_POINTS = [(rule, form, ema) for rule in RULES for form in FORMS for ema in (False, True)]


def _call(cl, rule, form, ema, null=(), n=8, tables=True, ngroups=1, rate=0.1):
    """The entry point of (rule, form, ema) with valid arguments, except: the pointers named in ``null`` are NULL, and ``n``,
    ``tables`` (False: both tables empty), ``ngroups`` and ``rate`` are what the caller says."""
    from clip_event_amd.optim import OptimGroup
    r = RULES[rule]
    name = f"ce_{rule}_step{FORMS[form]}" + ("_ema" if ema else "")
    args = [NULL if what in null else FAKE for what in ("p", "g", *r["state"], "p_bf16")]
    if form == "flat":
        args.append(c_long(n))
    else:
        args += [FAKE if tables else NULL, c_int(int(tables)), c_int(int(tables)), FAKE if tables else NULL, c_int(int(tables))]
    if form == "groups":
        groups = (OptimGroup * 9)(*[OptimGroup(0.1, 0.0, 0, 0) for _ in range(9)])
        args += [NULL, None, c_float(1.0), groups, c_int(ngroups), *r["grouped"]]          # segment_group, sumsq, max_norm, ...
    else:
        args += [None, c_float(1.0), *r["plain"]]
    if ema:
        args += [NULL if "ema" in null else FAKE, c_float(rate)]
    return name, getattr(cl, name)(*args, None)


def _cases(rule, form, ema):
    """(what is made invalid, a piece of the message it must produce)"""
    cases = [(dict(null=("p",)), b"null buffer"), (dict(null=("g",)), b"null buffer")]
    cases += [(dict(null=(s,)), RULES[rule]["null_state"]) for s in RULES[rule]["state"]]
    if form == "flat":
        cases += [(dict(n=0), b"n>0"), (dict(n=0, null=("p_bf16",)), b"n>0")]      # (the second: see the test's docstring)
    else:
        cases += [(dict(tables=False), b"nothing to update"), (dict(null=("p_bf16",)), b"null buffer")]
    if form == "groups":
        cases += [(dict(ngroups=0), b"groups"), (dict(ngroups=9), b"groups")]
    if ema:
        cases += [(dict(null=("ema",)), b"ema is NULL")] + [(dict(rate=bad), b"ema_rate") for bad in (0.0, 1.5, float("nan"))]
    return cases


@pytest.mark.parametrize("rule,form,ema", ENTRY_POINTS, ids=lambda v: {True: "ema", False: "plain"}.get(v, v))
def test_common_argument_errors_are_reported_without_a_gpu(rule, form, ema):
    """Every case returns -EINVAL and leaves a ``ce_last_error()`` that starts with the name of the entry point that was called
    (``ce_adam_step_ema:``, not its plain sibling's) and says what was wrong: n = 0 (flat) or empty tables (tiles, groups); NULL p,
    g, or state stream (Adam m and v -- refused like everyone else's since the checks are shared; SGD buf with momentum 0.9; Lion
    m); NULL p_bf16 in the table forms; ngroups 0 and 9; for the ``_ema`` twins NULL ema and ema_rate 0, 1.5, NaN.

    In the flat forms a NULL ``p_bf16`` is allowed (no mirror is written), so a call with it would launch on the fake pointers.
    It is not made: with n = 0 as well the ``n>0`` message wins, which is the documented order -- the form before the buffers --
    and the flat form's buffer check does not list ``p_bf16``."""
    from clip_event_amd._lib import lib
    cl = lib()
    for bad, msg in _cases(rule, form, ema):
        name, rc = _call(cl, rule, form, ema, **bad)
        assert rc == EINVAL, (name, bad, rc)
        err = cl.ce_last_error()
        assert err.startswith(name.encode() + b":") and msg in err, (name, bad, err)

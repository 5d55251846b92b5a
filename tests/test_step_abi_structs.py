"""CPU tests of the argument structs of the training step's launchers (include/idelucs_hip.h: idl_next_batch_t, idl_opt_tail_t, idl_opt_state_t): the ctypes
Structures of idelucs_amd/_lib.py mirror the C layout field for field, the launchers' refusals that involve the structs are reachable without a
device (every argument check stands before the first HIP call, so made-up addresses do), and the entry points the structs replaced are gone."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

from idelucs_amd import _lib

L = _lib.lib
HEADER = os.path.join(ROOT, "include", "idelucs_hip.h")
STRUCTS = {"idl_next_batch": _lib.idl_next_batch_t, "idl_opt_tail": _lib.idl_opt_tail_t, "idl_opt_state": _lib.idl_opt_state_t}


def _header_fields(tag):
    """The field names of `typedef struct <tag> { ... } <tag>_t;` in the header, in declaration order."""
    body = re.search(r"typedef struct %s \{(.*?)\} %s_t;" % (tag, tag), open(HEADER).read(), re.S).group(1)
    return [re.search(r"(\w+)\s*$", d).group(1) for decl in body.split(";") if decl.strip() for d in decl.split(",")]


def _c_compiler():
    for cc in (os.environ.get("CC"), "cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang", "/opt/rocm/lib/llvm/bin/clang"):
        if cc and shutil.which(cc):
            return shutil.which(cc)
    raise RuntimeError("no C compiler found (cc, gcc, clang): the header's layout cannot be checked")


def test_structures_mirror_the_header_layout(tmp_path):
    """A C program (C mode: the header stays includable from C) prints sizeof and every offsetof; ctypes must agree, in the header's field order."""
    fields = {tag: _header_fields(tag) for tag in STRUCTS}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "idelucs_hip.h"', "int main(void) {"]
    for tag, names in fields.items():
        lines.append('    printf("%s sizeof %%zu\\n", sizeof(%s_t));' % (tag, tag))
        lines += ['    printf("%s %s %%zu %%zu\\n", offsetof(%s_t, %s), sizeof(((%s_t *)0)->%s));' % (tag, f, tag, f, tag, f) for f in names]
    lines += ["    return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([_c_compiler(), "-x", "c", "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    seen = {tag: [] for tag in STRUCTS}
    for tag, name, *nums in (ln.split() for ln in out if ln):
        if name == "sizeof":
            assert ctypes.sizeof(STRUCTS[tag]) == int(nums[0]), tag
        else:
            seen[tag].append(name)
            field = getattr(STRUCTS[tag], name)
            assert (field.offset, field.size) == (int(nums[0]), int(nums[1])), (tag, name)
    for tag, S in STRUCTS.items():
        assert [n for n, _ in S._fields_] == fields[tag] == seen[tag], tag


# ---- refusals: made-up, suitably aligned device addresses; the host arrays of the tail are real (the launchers read them)
def _a(i):
    return ctypes.c_void_p(0x10000 * i)


N_T = 3
_PP = (ctypes.c_void_p * N_T)(0x100000, 0x200000, 0x300000)
_SZ = (ctypes.c_int64 * N_T)(512 * 128, 512, 64)
CTL = 0x400000


def _tail(**over):
    f = dict(count=N_T, params=_PP, grads=_PP, grad_parts=None, square_avg=_PP, sizes=_SZ, hyper=_a(5), ctl=ctypes.c_void_p(CTL), loss_rows=None,
             loss_m=0, w_nce=0.5, w_iic=0.5, out=_a(6), skip_index=-1, wg_index=-1, batch_advance=0)
    f.update(over)
    return _lib.idl_opt_tail_t(**f)


def _next_batch(**over):
    """A whole batch of 4 pairs from a 10 x 8 store, assembled at ctl[1] into fp32 rows: what idl_rmsprop_step takes."""
    f = dict(feats=_a(7), n=10, f=8, view_stride=80, pair_idx=_a(8), base=ctypes.c_void_p(CTL + 8), base_add=0, n_pairs=20, batch=4, mean=_a(9),
             scale=_a(10), inv_scale=None, y=_a(11), y_hi=None, y_lo=None, overflow_flag=None, part=0, part_end=8, parts=8)
    f.update(over)
    return _lib.idl_next_batch_t(**f)


def _refused(rc, text):
    assert rc == _lib.IDL_ERR_ARG and text in _lib.last_error(), (rc, _lib.last_error())


@pytest.mark.parametrize("over, text", [
    (dict(base=ctypes.c_void_p(CTL)), "next_batch->base must be ctl + 1"),
    (dict(y_hi=_a(12), y_lo=_a(13)), "writes no planes"),
    (dict(base_add=4), "takes no base_add"),
    (dict(part=4), "the whole batch, not a share"),
    (dict(part_end=4), "the whole batch, not a share"),
], ids=["base", "planes", "base_add", "share_tail", "share_head"])
def test_optimizer_launch_refuses_what_it_cannot_assemble(over, text):
    _refused(L.idl_rmsprop_step(_tail(), _next_batch(**over), None), text)


# ---- the opt-in last launches: idl_opt_step_gather_wgrad (NetLinear) and idl_small_wgrad_rms / _rms_momentum / _opt (model_size='small')
_P8 = (ctypes.c_void_p * 8)(*[0x100000 * (i + 1) for i in range(8)])
SMALL_F = 8           # _next_batch()'s row width: the small launch wants next_batch->f == F


def _opt_state(**over):
    """Adam on made-up states: valid for either family (state arrays of 8 entries; the linear launch reads the first N_T)."""
    f = dict(kind=2, state1=_P8, state2=_P8, hyper=_a(14), step_in=_a(15), step_out=ctypes.c_void_p(0x10000 * 15 + 8))
    f.update(over)
    return _lib.idl_opt_state_t(**f)


def _linear_opt(nb=None, opt=None, **tail):
    return L.idl_opt_step_gather_wgrad(_tail(**{"square_avg": None, "hyper": None, **tail}), opt if opt is not None else _opt_state(), nb, None)


def _small_from_x(nb):
    return [_a(i) for i in range(20, 28)] + [4, SMALL_F, 5, None, 0.5, 0.5, None, nb, None]


def _small_rms(nb=None, opt=None):
    return L.idl_small_wgrad_rms(_P8, None, _P8, _a(5), ctypes.c_void_p(CTL), *_small_from_x(nb))


def _small_momentum(nb=None, opt=None):
    return L.idl_small_wgrad_rms_momentum(_P8, None, _P8, _P8, _a(5), ctypes.c_void_p(CTL), *_small_from_x(nb))


def _small_opt(nb=None, opt=None):
    return L.idl_small_wgrad_opt(opt if opt is not None else _opt_state(), _P8, None, ctypes.c_void_p(CTL), *_small_from_x(nb))


LAST_LAUNCHES = {"opt_step_gather_wgrad": _linear_opt, "small_wgrad_rms": _small_rms, "small_wgrad_rms_momentum": _small_momentum,
                 "small_wgrad_opt": _small_opt}


@pytest.mark.parametrize("over, text", [
    (dict(base=ctypes.c_void_p(CTL)), "next_batch->base must be ctl + 1"),
    (dict(y_hi=_a(12), y_lo=_a(13)), "writes no planes"),
    (dict(base_add=4), "takes no base_add"),
    (dict(part=4), "the whole batch, not a share"),
    (dict(part_end=4), "the whole batch, not a share"),
], ids=["base", "planes", "base_add", "share_tail", "share_head"])
@pytest.mark.parametrize("entry", sorted(LAST_LAUNCHES))
def test_opt_in_last_launches_refuse_what_the_optimizer_launch_refuses(entry, over, text):
    """The whole-batch rules of idl_rmsprop_step hold for every last launch that assembles the next batch (csrc/step_args.h: one text)."""
    _refused(LAST_LAUNCHES[entry](nb=_next_batch(**over)), text)


OPT_STATE_REFUSALS = [
    (dict(kind=0), "opt->kind is 1"),
    (dict(state2=None), "opt->state2 for Adam"),
    (dict(hyper=ctypes.c_void_p(0xE0004)), "opt->hyper is a device double[5]"),
    (dict(step_out=_a(15)), "read from one word and written to another"),
    (dict(step_in=ctypes.c_void_p(CTL)), "opt->step_in must not be a word this launch writes"),
    (dict(step_in=ctypes.c_void_p(CTL + 8)), "opt->step_in must not be a word this launch writes"),
]
OPT_STATE_IDS = ["kind_0", "adam_without_state2", "hyper_misaligned", "one_step_word", "step_in_is_ctl0", "step_in_is_ctl1"]


@pytest.mark.parametrize("over, text", OPT_STATE_REFUSALS, ids=OPT_STATE_IDS)
@pytest.mark.parametrize("entry", ["opt_step_gather_wgrad", "small_wgrad_opt"])
def test_optimizer_state_refusals(entry, over, text):
    """The optimizer-state rules, one text for both families (csrc/step_args.h opt_state_of); a refusal names the field."""
    _refused(LAST_LAUNCHES[entry](opt=_opt_state(**over)), text)


def test_small_wgrad_opt_takes_no_rmsprop():
    _refused(_small_opt(opt=_opt_state(kind=3)), "opt->kind is 1 (SGD with momentum) or 2 (Adam)")


@pytest.mark.parametrize("kw, text", [
    (dict(square_avg=_PP), "tail->square_avg and tail->hyper must be NULL"),
    (dict(skip_index=0), "tail->skip_index must be -1"),
    (dict(nb=True, batch_advance=4), "tail->batch_advance must be 0"),
], ids=["square_avg", "skip_index", "advance_beside_assembly"])
def test_opt_step_gather_wgrad_refuses_what_the_tail_cannot_mean(kw, text):
    """The tail's RMSprop fields are empty beside an idl_opt_state_t, and the launch that assembles the next batch reads ctl[1]: it cannot advance it."""
    if kw.get("nb"):
        kw = dict(kw, nb=_next_batch())
    _refused(_linear_opt(**kw), text)


LAST_LAUNCH_ENTRIES = ("idl_opt_step_gather_wgrad", "idl_small_wgrad_rms", "idl_small_wgrad_rms_momentum", "idl_small_wgrad_opt")


def test_last_launch_entries_stay_short():
    """No last-launch entry takes more than 24 arguments.  They took 32 to 38 while the next batch's assembly travelled as eleven loose values, in
    an order that differed between the two families in two int64 places: a swap there compiles, links and runs.  The assembly and the
    optimizer's state are structs now (named fields, one check each); a signature that grows past 24 is that list coming back."""
    for name in LAST_LAUNCH_ENTRIES:
        assert len(_lib.SIGNATURES[name][1]) <= 24, name
    nb, opt = ctypes.POINTER(_lib.idl_next_batch_t), ctypes.POINTER(_lib.idl_opt_state_t)
    assert all(_lib.SIGNATURES[name][1][-2] == nb for name in LAST_LAUNCH_ENTRIES)
    assert _lib.SIGNATURES["idl_opt_step_gather_wgrad"][1][1] == opt and _lib.SIGNATURES["idl_small_wgrad_opt"][1][0] == opt


def test_mid_bwd_gather_needs_the_dr1_flag_with_dr1_planes():
    p = [_a(i) for i in range(1, 20)]
    rc = L.idl_mid_bwd_gather(p[0], p[1], p[2], p[3], p[4], 1, p[5], p[6], p[7], p[8], 32, 10, 1, 1e-3, p[9], p[10], None, p[11], p[12], p[13], p[14], 1,
                              p[15], p[16], p[17], None, None, None, None)
    _refused(rc, "dr1's planes need both planes (16-byte aligned), the words of their scale and the flag")


def test_mid_fwd_gather_needs_both_planes_of_the_next_batch():
    p = [_a(i) for i in range(1, 12)]
    nb = _next_batch(base_add=4, y_hi=_a(12), part_end=4)
    rc = L.idl_mid_fwd_gather(p[0], None, 0, p[1], p[2], p[3], p[4], 32, 10, 1, 3, p[5], p[6], p[7], p[8], p[9], nb, None)
    _refused(rc, "mid_fwd_gather: both planes of the next batch (8-byte aligned) or neither")


def test_reduce_parts_rms_takes_no_snapshot_beside_a_tail():
    rc = L.idl_reduce_parts_rms(_a(1), 512 * 128, _a(2), _a(3), _tail(skip_index=0), None)
    _refused(rc, "the step counter's snapshot needs both pointers and a launch without the tail")


@pytest.mark.parametrize("skip", [-1, N_T])
def test_wgrad_rmsprop_step_needs_its_tensor(skip):
    rc = L.idl_wgrad_rmsprop_step(_a(1), _a(2), 128, 512, 128, None, _tail(skip_index=skip), None)
    _refused(rc, "wgrad_rmsprop_step: skip_index outside the tensors")


def test_replaced_entry_points_are_gone():
    hdr = open(HEADER).read()
    for name in ("idl_mid_fwd_gather_planes", "idl_mid_bwd_gather_planes", "idl_rmsprop_step_gather", "idl_rmsprop_step_gather_wgrad"):
        assert not re.search(r"\b%s\b" % name, hdr), name
        assert name not in _lib.SIGNATURES
        assert not hasattr(L, name), f"{name} is still exported"

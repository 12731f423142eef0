"""The host layer of the evaluation bindings (mlp_eval_gen,
mlp_eval_reg_gen): each precondition broken alone is refused before
anything is launched, and every buffer stays as it was.

As in tests/test_gpu_host_layer.py, no case relies on a kernel reading out
of bounds to be noticed: an undersized argument is a leading slice of a
full-sized allocation, a wrong dtype a reinterpreting view of one, a
misaligned one an offset view into a larger one."""

import pytest
import torch

pytestmark = pytest.mark.gpu

NAN = float("nan")
B = 150            # two workgroups at RT = 128


@pytest.fixture(scope="module")
def ext():
    from unionml_amd.ops import hip_ext

    if not torch.cuda.is_available():
        pytest.skip("needs MI355X")
    return hip_ext(required=True)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def good_args(ext, dev, regression):
    """A valid call's arguments by name, geometry 70x50x7 -> <64,128,16>"""
    from unionml_amd.ops.tabular import TabularMLP, TabularMLPRegressor

    model = (TabularMLPRegressor if regression else TabularMLP)(70, 50, 7, device=dev, seed=1)
    g = model.g
    gen = torch.Generator().manual_seed(0)
    rec = ext.eval_rec_reg_n(g.cpad) if regression else ext.EVAL_REC_CLS_N
    if regression:
        tgt = torch.zeros(B, g.cpad)
        tgt[:, :7] = torch.randn(B, 7, generator=gen)
    else:
        tgt = (torch.arange(B) % 7).int()
    a = dict(
        Xbf=torch.randn(B, g.inp, generator=gen).bfloat16().to(dev),
        tgt=tgt.to(dev), hid=g.hid, n_out=7, wimg=model.wimg, master=model.master,
        part=torch.full((2, rec), NAN, device=dev),
        hist=torch.full((2, rec), NAN, device=dev),
        slot=torch.zeros(1, dtype=torch.int32, device=dev),
    )
    return model, a, rec


def call(ext, regression, a):
    fn = ext.mlp_eval_reg_gen if regression else ext.mlp_eval_gen
    fn(a["Xbf"], a["tgt"], a["hid"], a["n_out"], a["wimg"], a["master"], a["part"],
       a["hist"], a["slot"])


def misaligned(t):
    """The same values at an address 2 (bf16) or 4 (fp32) bytes off 16"""
    big = torch.zeros(t.numel() + 8, dtype=t.dtype, device=t.device)
    view = big[1 : 1 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    return view


def breakers(regression, rec):
    """name -> function that breaks exactly one precondition of ``a``"""
    out = {
        "Xbf on the host": lambda a: a.update(Xbf=a["Xbf"].cpu()),
        "Xbf not contiguous": lambda a: a.update(Xbf=a["Xbf"].t().contiguous().t()),
        "Xbf wrong dtype": lambda a: a.update(Xbf=a["Xbf"].view(torch.float16)),
        "Xbf not 2-d": lambda a: a.update(Xbf=a["Xbf"].view(-1)),
        "Xbf empty": lambda a: a.update(Xbf=a["Xbf"][:0], tgt=a["tgt"][:0]),
        "Xbf misaligned": lambda a: a.update(Xbf=misaligned(a["Xbf"])),
        "inp not a multiple of 32": lambda a: a.update(Xbf=a["Xbf"][:, :80].contiguous()),
        "wimg misaligned": lambda a: a.update(wimg=misaligned(a["wimg"])),
        "wimg too short": lambda a: a.update(wimg=a["wimg"][:-1]),
        "wimg wrong dtype": lambda a: a.update(wimg=a["wimg"].view(torch.float16)),
        "master too short": lambda a: a.update(master=a["master"][:-1]),
        "master wrong dtype": lambda a: a.update(master=a["master"].view(torch.int32)),
        "targets too few": lambda a: a.update(tgt=a["tgt"][:-1]),
        "targets on the host": lambda a: a.update(tgt=a["tgt"].cpu()),
        "part too few rows": lambda a: a.update(part=a["part"][:1]),
        "part too narrow": lambda a: a.update(part=a["part"][:, : rec - 1].contiguous()),
        "part wrong dtype": lambda a: a.update(part=a["part"].view(torch.int32)),
        "part not 2-d": lambda a: a.update(part=a["part"].view(-1)),
        "hist no rows": lambda a: a.update(hist=a["hist"][:0]),
        "hist too narrow": lambda a: a.update(hist=a["hist"][:, : rec - 1].contiguous()),
        "hist not contiguous": lambda a: a.update(hist=a["hist"].t().contiguous().t()),
        "hist wrong dtype": lambda a: a.update(hist=a["hist"].view(torch.int32)),
        "slot wrong dtype": lambda a: a.update(slot=a["slot"].view(torch.float32)),
        "slot empty": lambda a: a.update(slot=a["slot"][:0]),
        "slot on the host": lambda a: a.update(slot=a["slot"].cpu()),
        "n_out zero": lambda a: a.update(n_out=0),
        "n_out 33": lambda a: a.update(n_out=33),
        "hid without an instantiation": lambda a: a.update(hid=48),
        "hid zero": lambda a: a.update(hid=0),
    }
    if regression:
        out["Yt wrong width"] = lambda a: a.update(tgt=a["tgt"][:, :7].contiguous())
        out["Yt wrong dtype"] = lambda a: a.update(tgt=a["tgt"].view(torch.int32))
        out["Yt misaligned"] = lambda a: a.update(tgt=misaligned(a["tgt"]))
        out["Yt not 2-d"] = lambda a: a.update(tgt=a["tgt"].view(-1))
    else:
        out["labels wrong dtype"] = lambda a: a.update(tgt=a["tgt"].long())
        out["labels too many"] = lambda a: a.update(
            tgt=torch.zeros(B + 1, dtype=torch.int32, device=a["tgt"].device))
    return out


NAMES = {r: sorted(breakers(r, 2)) for r in (False, True)}
CASES = [(r, n) for r in (False, True) for n in NAMES[r]]


@pytest.mark.parametrize("regression,name", CASES,
                         ids=[("reg-" if r else "clf-") + n.replace(" ", "_") for r, n in CASES])
def test_broken_precondition_is_refused(ext, dev, regression, name):
    model, a, rec = good_args(ext, dev, regression)
    watched = {k: a[k] for k in ("part", "hist", "slot")}
    before = {k: v.clone() for k, v in watched.items()}
    master = model.master.clone()
    breakers(regression, rec)[name](a)
    with pytest.raises((RuntimeError, TypeError)):
        call(ext, regression, a)
    torch.cuda.synchronize()
    for k, v in watched.items():
        assert torch.equal(v.view(torch.int32), before[k].view(torch.int32)), f"{k} was touched"
    assert torch.equal(model.master, master)


@pytest.mark.parametrize("regression", [False, True], ids=["clf", "reg"])
def test_the_unbroken_call_runs(ext, dev, regression):
    """... so the refusals above are the broken argument's doing."""
    _, a, rec = good_args(ext, dev, regression)
    call(ext, regression, a)
    torch.cuda.synchronize()
    assert torch.isfinite(a["part"]).all() and int(a["slot"].item()) == 1
    assert torch.isfinite(a["hist"][0, :1]).all() and torch.isnan(a["hist"][1]).all()

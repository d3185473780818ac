"""Generate the symplectic-flow golden vectors under tests/golden/ from the reference's own code.

Run ONLY in the authoring container (needs the reference checkout at /root/reference):

    python tests/golden/make_golden_symplectic.py

As in make_golden.py, ``torchdiffeq`` (imported by the reference at module import time) is bound to a placeholder that
raises if called: ``SymplecticFlowModel.log_prob`` goes through ``odeint`` and is NOT pinned here (the GPU tests anchor
it against scipy's solve_ivp and a closed-form flow instead).  Recorded: the weights, ``SymplecticMLP.forward`` at a
scalar and a per-row time, ``SymplecticFlowModel.sample`` with its captured prior for num_steps 1, 4 and 25 (shift /
scale and conditional shift / scale not the identity), the ``state_dict`` key lists and the signatures of the public
methods.  Only numbers and names are stored (.npz); no reference source is copied.
"""
import inspect
import json
import sys
import types
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent

# name: (n_data_dims, n_conditionals, embedding_dimensions, units); the last one is outside the compiled pair kernels
CASES = {
    "sym_2d": (2, 0, 8, [64, 64]),
    "sym_16d_2x256": (16, 0, 16, [256, 256]),
    "sym_5d_c3_ragged": (5, 3, 6, [100, 128]),
    "sym_20d_outside": (20, 0, 8, [64]),
}
STEPS = (1, 4, 25)


def _import_reference():
    def _absent(*a, **k):
        raise RuntimeError("torchdiffeq is not available offline; this code path is not pinned")
    stub = types.ModuleType("torchdiffeq")
    stub.odeint = _absent
    stub.odeint_adjoint = _absent
    sys.modules.setdefault("torchdiffeq", stub)
    sys.path.insert(0, "/root/reference")
    import flowfusion.symplectic as rs
    return rs


def _save(name, meta, **arrays):
    out = {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in arrays.items()}
    out["__meta__"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    np.savez_compressed(HERE / f"{name}.npz", **out)
    print(f"wrote {name}.npz  ({(HERE / f'{name}.npz').stat().st_size / 1024:.0f} KiB)")


def main():
    rs = _import_reference()
    sigs = {
        "SymplecticMLP.__init__": str(inspect.signature(rs.SymplecticMLP.__init__)),
        "SymplecticMLP.forward": str(inspect.signature(rs.SymplecticMLP.forward)),
        "SymplecticFlowModel.__init__": str(inspect.signature(rs.SymplecticFlowModel.__init__)),
        "SymplecticFlowModel.sample": str(inspect.signature(rs.SymplecticFlowModel.sample)),
        "SymplecticFlowModel.log_prob": str(inspect.signature(rs.SymplecticFlowModel.log_prob)),
    }
    for i, (name, (D, C, E, units)) in enumerate(CASES.items()):
        torch.manual_seed(700 + i)
        m = rs.SymplecticMLP(D, C, E, units)
        shift, scale = torch.randn(D) * 0.5, torch.rand(D) + 0.5
        cshift = torch.randn(C) * 0.5 if C else None
        cscale = torch.rand(C) + 0.5 if C else None
        model = rs.SymplecticFlowModel(m, shift, scale, cshift, cscale)
        B = 24
        state = torch.randn(B, 2 * D)
        cond = torch.randn(B, C) if C else None
        cond_n = (cond - cshift) / cscale if C else None
        tv = torch.rand(B)
        ts = torch.tensor(0.37)
        with torch.no_grad():
            out_v = m(tv, state, cond_n)
            out_s = m(ts, state, cond_n)
        arrays = dict(state=state, t_vec=tv, t_scalar=ts, fwd_vec=out_v, fwd_scalar=out_s)
        if C:
            arrays["cond"] = cond
        for n in STEPS:
            torch.manual_seed(900 + n)
            arrays[f"prior_{n}"] = torch.randn(B, 2 * D)          # what sample() draws first (symplectic.py:188)
            torch.manual_seed(900 + n)
            arrays[f"sample_{n}"] = model.sample((B, D), conditional=cond, num_steps=n)
        for k, v in model.state_dict().items():
            arrays["sd." + k] = v
        meta = dict(D=D, C=C, E=E, units=units, steps=list(STEPS), state_dict_keys=list(model.state_dict().keys()),
                    mlp_state_dict_keys=list(m.state_dict().keys()), signatures=sigs)
        _save(name, meta, **arrays)


if __name__ == "__main__":
    main()

"""Float64 restatement of the symplectic flow (reference flowfusion/symplectic.py) for the tests, from a ``state_dict``:
the dynamics, the Euler sampler on the reference's grid, and the log-density integrated by scipy's ``solve_ivp`` (to
convergence) or by torchdiffeq's dopri5 step control (the oracle's float64 restatement); known-answer weights."""
import math

import torch


class SymplecticRef:
    """``SymplecticFlowModel`` in float64 on the CPU.  ``sd``: the model's state_dict (keys ``shift``, ``scale``,
    [``conditional_shift``, ``conditional_scale``,] ``model.W``, ``model.mlp_{q,p}_dynamics.{i}.{weight,bias}``)."""

    def __init__(self, sd):
        f64 = lambda k: sd[k].detach().to("cpu", torch.float64)
        self.W = f64("model.W")
        self.shift, self.scale = f64("shift"), f64("scale")
        self.cshift = f64("conditional_shift") if "conditional_shift" in sd else None
        self.cscale = f64("conditional_scale") if "conditional_scale" in sd else None
        self.nets = []
        for name in ("mlp_q_dynamics", "mlp_p_dynamics"):
            idx = sorted({int(k.split(".")[2]) for k in sd if k.startswith(f"model.{name}.")})
            self.nets.append([(f64(f"model.{name}.{i}.weight"), f64(f"model.{name}.{i}.bias")) for i in idx])

    @staticmethod
    def _mlp(layers, h):
        for i, (w, b) in enumerate(layers):
            h = h @ w.T + b
            if i < len(layers) - 1:
                h = h * torch.sigmoid(h)
        return h

    def norm_cond(self, cond):
        return None if cond is None else (cond.double() - self.cshift) / self.cscale

    def forward(self, t, state, cond_n=None):
        """v = [mlp_q([p, cond, emb]), -mlp_p([q, cond, emb])], emb = [sin | cos](t W 2 pi); ``cond_n`` normalised."""
        state = state.double()
        q, p = state.chunk(2, dim=-1)
        t = torch.as_tensor(t, dtype=torch.float64)
        if t.dim() == 0:
            t = t.expand(q.shape[0])
        arg = t[:, None] * self.W[None, :] * 2 * math.pi
        emb = torch.cat([torch.sin(arg), torch.cos(arg)], dim=1)
        extra = [cond_n.double()] if cond_n is not None else []
        vq = self._mlp(self.nets[0], torch.cat([p] + extra + [emb], dim=1))
        vp = -self._mlp(self.nets[1], torch.cat([q] + extra + [emb], dim=1))
        return torch.cat([vq, vp], dim=-1)

    def sample_from(self, prior, cond=None, num_steps=1):
        """The reference's Euler loop on the fp32 grid linspace(1, 0, num_steps + 1), in float64."""
        cond_n = self.norm_cond(cond)
        ts = torch.linspace(1.0, 0.0, num_steps + 1)
        x = prior.double()
        for i in range(num_steps):
            dt = float(ts[i + 1] - ts[i])
            x = x + self.forward(float(ts[i]), x, cond_n) * dt
        q = x.chunk(2, dim=-1)[0]
        return q * self.scale + self.shift

    def _log_prob(self, x, p0, cond, solve):
        cond_n = self.norm_cond(cond)
        q0 = (x.double() - self.shift) / self.scale
        z1 = solve(torch.cat([q0, p0.double()], dim=-1), cond_n)
        logn = lambda z: (-0.5 * z ** 2 - 0.5 * math.log(2 * math.pi)).sum(-1)
        return logn(z1) - logn(p0.double()) - torch.log(self.scale).sum()

    def log_prob_from(self, x, p0, cond=None, rtol=1e-10, atol=1e-12):
        """log N(z1) - log N(p0) - sum log scale with z1 from scipy's RK45 run to convergence."""
        from scipy.integrate import solve_ivp

        def solve(z0, cond_n):
            B, D2 = z0.shape

            def f(t, y):
                return self.forward(float(t), torch.from_numpy(y.reshape(B, D2).copy()), cond_n).reshape(-1).numpy()
            sol = solve_ivp(f, (0.0, 1.0), z0.reshape(-1).numpy(), method="RK45", rtol=rtol, atol=atol)
            assert sol.success
            return torch.from_numpy(sol.y[:, -1].reshape(B, D2))
        return self._log_prob(x, p0, cond, solve)

    def log_prob_dopri5(self, x, p0, cond=None, tol=1e-5):
        """The same with z1 from torchdiffeq's dopri5 at rtol = atol = tol, in float64 (the oracle's restatement of its
        step control, oracle/flowfusion_oracle.py odeint_dopri5): what the reference's log_prob computes, up to fp32."""
        from oracle import flowfusion_oracle as O

        def solve(z0, cond_n):
            f = lambda t, ys: (self.forward(t.double(), ys[0], cond_n),)
            return O.odeint_dopri5(f, (z0,), torch.tensor([0.0, 1.0]), rtol=tol, atol=tol)[0]
        return self._log_prob(x, p0, cond, solve)


def rotation_weights(D, C, E, units, alpha, beta):
    """Known-answer weights (float32 state_dict entries of a SymplecticMLP): with SiLU(x) - SiLU(-x) = x every depth of
    first layer [I; -I], hidden layers [[I, -I], [-I, I]] and output [I, -I] gives mlp_q = alpha p, mlp_p = beta q, so
    v = [alpha p, -beta q]; spare hidden units, conditional and time columns are zero."""
    sd = {}
    for name, s in (("mlp_q_dynamics", alpha), ("mlp_p_dynamics", beta)):
        n_in = D + C + E
        sizes = [n_in] + list(units) + [D]
        for li in range(len(sizes) - 1):
            w = torch.zeros(sizes[li + 1], sizes[li])
            eye = torch.eye(D)
            if li == 0:
                w[:D, :D], w[D:2 * D, :D] = eye, -eye
            elif li < len(sizes) - 2:
                w[:D, :D], w[:D, D:2 * D], w[D:2 * D, :D], w[D:2 * D, D:2 * D] = eye, -eye, -eye, eye
            else:
                w[:, :D], w[:, D:2 * D] = s * eye, -s * eye
            sd[f"{name}.{2 * li}.weight"] = w
            sd[f"{name}.{2 * li}.bias"] = torch.zeros(sizes[li + 1])
    return sd


def euler_rotation(prior, D, alpha, beta, num_steps):
    """Product of the Euler matrices (I + dt_k A), A = [[0, alpha I], [-beta I, 0]], on the fp32 grid, in float64."""
    ts = torch.linspace(1.0, 0.0, num_steps + 1)
    z = prior.double()
    for i in range(num_steps):
        dt = float(ts[i + 1] - ts[i])
        q, p = z[:, :D], z[:, D:]
        z = torch.cat([q + dt * alpha * p, p - dt * beta * q], dim=1)
    return z

"""CPU: the float64 oracles against closed forms in 50-digit arithmetic at the activation edge probes
(tests/activation_probes.py).  This is what licenses the float64 oracle as the reference of tests/test_gpu_activation_edges.py:
at every probe, for every activation, it is within 1e-14 max(1, |ref|) of the exact value -- two orders below the tightest
device bar (1e-12)."""
import numpy as np
import pytest

import activation_probes as ap
from oracle import nempc_oracle as orc

SPECS = ap.ACTS + ("elu", "leaky_relu")        # the parameterised ones at their defaults, too
BOUND = 1e-14


def _mp_close(got, ref, what):
    import mpmath as mp
    assert np.isfinite(got), what
    err = abs(mp.mpf(float(got)) - ref)
    lim = BOUND * max(mp.mpf(1), abs(ref))
    assert err <= lim, f"{what}: oracle {float(got)!r}, closed form {mp.nstr(ref, 20)}, error {mp.nstr(err, 3)} > {mp.nstr(lim, 3)}"
    return float(err / max(mp.mpf(1), abs(ref)))


@pytest.mark.parametrize("spec", SPECS)
def test_oracle_activation_formulas_against_closed_forms(spec):
    z = ap.probes(spec)
    with np.errstate(over="ignore"):
        a = orc.act_f(spec, z)
        s1, s2 = orc.act_s1(spec, z, a), orc.act_s2(spec, z, a)
    worst = 0.0
    for i, zi in enumerate(z):
        ref = ap.closed_form(spec, zi)
        for got, r, what in ((a[i], ref[0], "s"), (s1[i], ref[1], "s'"), (s2[i], ref[2], "s''")):
            worst = max(worst, _mp_close(got, r, f"{spec} {what}({zi!r})"))
    print(f"{spec}: worst oracle error against the closed forms {worst:.2e}")


def test_closed_forms_follow_the_tensorflow_conventions_at_the_kinks():
    for z0 in (0.0, -0.0):
        assert ap.closed_form("relu", z0)[1] == 0
        assert ap.closed_form("elu:0.5", z0)[1] == 0.5 and ap.closed_form("elu", z0)[1] == 1
        assert ap.closed_form("leaky_relu:0.1", z0)[1] == ap.closed_form("leaky_relu:0.1", -1.0)[1]
        assert ap.closed_form("relu6", z0)[1] == 0
        assert ap.closed_form("softsign", z0)[2] == 0
    assert ap.closed_form("relu6", 6.0)[1] == 0 and ap.closed_form("relu6", 5.999999)[1] == 1


def test_probe_table_holds_what_it_must():
    z = ap.PROBES
    for v in (0.0, 2.0 ** -60, 1e-300, 0.17, 0.1733, 0.3465, 1.0, 9.999, 10.001, 19.999, 20.0, 20.001, 36.7, 40.0, 88.8, 103.0,
              700.0, 709.7, 745.0, 800.0, 1024.0, 1100.0):
        assert v in z and -v in z, v
    assert np.signbit(z[z == 0.0]).tolist() == [False, True]
    for v in (-0.3466, 5.999999, 6.0, 6.000001):
        assert v in z
    assert np.isfinite(z).all() and z.size <= ap.B * ap.H and (ap.B * ap.H) % 16 != 0
    assert ap.probes("exponential").max() == 40.0 and ap.probes("exponential").min() == ap.N_WRAP
    assert np.sort(np.abs(z))[-2] == 1100.0 and round(ap.N_WRAP / np.log(2.0)) == -2 ** 32
    z32 = ap.probes("tanh", np.float32)
    assert z32[4] == 0.0 and z32[5] == 0.0 and 19.999 not in z32       # what float32 makes of 1e-300 and of 19.999


def _nets(spec, p):
    yield "one", ap.probe_net([spec, "linear"], p), 0
    yield "two", ap.probe_net(["linear", spec, "linear"], p, widths=(ap.WIDTH, ap.WIDTH)), 1


@pytest.mark.parametrize("p", [0, ap.WIDTH - 1])
@pytest.mark.parametrize("spec", SPECS)
def test_oracle_problem_on_the_probe_network_against_closed_forms(spec, p):
    """The isolating Jacobian column and the (u_t, u_t) Lagrangian entry of orc.Problem -- and of the C oracle, which
    evaluates the same activations with libm -- are [1, -0.5] s'(z*) and sigma 2 R + (lam_t . [1, -0.5]) s''(z*)."""
    import mpmath as mp
    from oracle.c_oracle import COracle
    Z, X0, lam, _, sigma = ap.probe_inputs(spec)
    z = ap.probes(spec)
    ref = [ap.closed_form(spec, zi) for zi in z]
    worst = 0.0
    for variant, net, layer in _nets(spec, p):
        for w in net.W + net.b:
            assert np.array_equal(w.astype(np.float32).astype(np.float64), w)     # the fp32 runs see the same network
        prob = ap.probe_problem(net)
        with np.errstate(over="ignore"):
            jac = np.stack([prob.jacobian(Z[i], X0[i]) for i in range(ap.B)])
            hd = np.stack([prob.lagrangian_hessian(Z[i], X0[i], lam[i], sigma[i]) for i in range(ap.B)])
            cjac = COracle(prob).eval(Z, X0)[3]
        assert np.isfinite(jac).all() and np.isfinite(hd).all() and np.isfinite(cjac).all()
        col, ccol, huu = ap.isolating_column(jac), ap.isolating_column(cjac), ap.uu_entry(hd)
        # the probe unit's pre-activation is u_t bit for bit
        u = Z[:, ap.H * ap.NX:].reshape(-1, 1)
        xprev = np.concatenate([X0[:, None, :], Z[:, :ap.H * ap.NX].reshape(ap.B, ap.H, ap.NX)[:, :-1]], axis=1).reshape(-1, ap.NX)
        zs = net._acts(np.concatenate([xprev, u], axis=1), with_z=True)[1]
        # (as a value: the sum with the zero products and the zero bias turns the probe -0.0 into +0.0, here and on the device)
        assert np.array_equal(zs[layer][:, p], u[:, 0])
        assert np.array_equal(u[:z.size, 0], z) and np.all(u[z.size:] == ap.SPARE)
        for i in range(z.size):
            bi, t = ap.stage_of_probe(i)
            for k in range(ap.NX):
                worst = max(worst, _mp_close(col[i, k], mp.mpf(ap.OUT_ROW[k]) * ref[i][1], f"{spec}/{variant} column, probe {z[i]!r}"))
                _mp_close(ccol[i, k], mp.mpf(ap.OUT_ROW[k]) * ref[i][1], f"{spec}/{variant} C oracle column, probe {z[i]!r}")
            lt = lam[bi, t * ap.NX:(t + 1) * ap.NX]
            exact = mp.mpf(sigma[bi]) * 2 * ap.R_WEIGHT + mp.mpf(float(lt @ ap.OUT_ROW)) * ref[i][2]
            worst = max(worst, _mp_close(huu[i], exact, f"{spec}/{variant} (u, u) entry, probe {z[i]!r}"))
    print(f"{spec} p={p}: worst isolating-column / (u, u) error of the oracle {worst:.2e}")

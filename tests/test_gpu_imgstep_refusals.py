"""The argument rules of the seven image steps around the beamformer -- pulse, envelope, log compression, axial FIR, rf2iq, I/Q
envelope, scan conversion -- as their fourteen entry points keep them (csrc/img_request.h; the whole table, boundaries and launch
shapes are held on the CPU by tests/test_img_request_host.py).  Through ctypes, on shapes of a few elements: for either form of a
step one case per rule, the null context, an accepted call and every empty call, each with its return code as a literal; then, with
a recording open, every host form is refused by the context and an empty host call still returns 0.  A refused or empty call touches
no buffer, so the out-of-range cases pass the same 64-float buffers as the accepted ones."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NX, NZ, NT, T = 2, 8, 2, 16
ENV_MAX_N, FIR_MAX_K, RF2IQ_MAX_D = 4096, 1024, 8
NAN, INF = float("nan"), float("inf")
BUFS = ("a", "b", "taps", "x", "z")


class Form:
    """one form of the entry points: the "_dev" suffix or none, and five disjoint 64-float buffers of its kind"""

    def __init__(self, mi, ctx, dev):
        self.ctx, self.lib, self.dev = ctx, ctx.lib, dev
        fill = np.linspace(0.5, 1.5, 64, dtype=np.float32)
        self.keep = {k: (mi.DeviceBuffer.from_host(ctx, fill) if dev else fill.copy()) for k in BUFS}

    def p(self, name):
        if name is None:
            return None
        b = self.keep[name]
        return int(b.ptr) if self.dev else b.ctypes.data

    def call(self, name, *args, handle=True):
        return getattr(self.lib, name + ("_dev" if self.dev else ""))(self.ctx.handle if handle else None, *args)

    def close(self):
        if self.dev:
            for b in self.keep.values():
                b.close()


@pytest.fixture(scope="module")
def forms(mi):
    ctx = mi.Context()
    f = {"host": Form(mi, ctx, False), "dev": Form(mi, ctx, True)}
    yield f
    for v in f.values():
        v.close()
    ctx.close()


def pulse(L, nt=NT, T=T, fs=40e6, f=5e6, sigma=1e-7, i="a", o="b", **kw):     # K = ceil(2.5 sigma fs) = 10
    return L.call("pbrt_us_apply_pulse", nt, T, fs, f, sigma, L.p(i), L.p(o), **kw)


def envelope(L, nx=NX, nz=NZ, i="a", o="b", **kw):
    return L.call("pbrt_envelope", nx, nz, L.p(i), L.p(o), **kw)


def log_compress(L, n=NX * NZ, dr=50.0, i="a", o="b", **kw):
    return L.call("pbrt_log_compress", n, L.p(i), dr, L.p(o), **kw)


def axial_fir(L, nx=NX, nz=NZ, K=2, taps="taps", i="a", o="b", **kw):
    return L.call("pbrt_axial_fir", nx, nz, K, L.p(taps), L.p(i), L.p(o), **kw)


def rf2iq(L, nt=NT, T=T, fs=40e6, t0=0.0, fd=5e6, D=2, K=2, taps="taps", i="a", o="b", **kw):
    return L.call("pbrt_rf2iq", nt, T, fs, t0, fd, D, K, L.p(taps), L.p(i), L.p(o), **kw)


def iq_envelope(L, n=NX * NZ, i="a", o="b", **kw):
    return L.call("pbrt_iq_envelope", n, L.p(i), L.p(o), **kw)


def scan_convert(L, capi=None, null_params=False, src="a", x="x", z="z", dst="b", handle=True, **edits):
    p = capi.ScanConvertParams(n_theta=4, n_rho=4, nx=NX, nz=NZ, theta0=-0.3, dtheta=0.2, rho0=0.01, drho=0.01, ox=0.0, oz=0.0, fill=0.0)
    for k, v in edits.items():
        setattr(p, k, v)
    return L.call("pbrt_scan_convert", None if null_params else C.byref(p), L.p(src), L.p(x), L.p(z), L.p(dst), handle=handle)


# step -> [(arguments that differ from the accepted call, return code of the host form, of the _dev form)]
CASES = {
    pulse: [
        (dict(), 0, 0),
        (dict(i=None), -1, -1), (dict(o=None), -1, -1), (dict(o="a"), -1, -1),
        (dict(fs=0.0), -1, -1), (dict(fs=NAN), -1, -1), (dict(f=0.0), -1, -1), (dict(sigma=0.0), -1, -1), (dict(sigma=-1e-7), -1, -1),
        (dict(nt=65536), -1, -1), (dict(nt=65535, T=65537), -1, -1),          # the second grid dimension; 2^32 - 1 samples
        (dict(sigma=1.0, fs=1000.0), -1, -1),                                # K = 2500 > PULSE_MAX_K
        (dict(nt=0), 0, 0), (dict(T=0), 0, 0), (dict(nt=0, T=0), 0, 0),
    ],
    envelope: [
        (dict(), 0, 0),
        (dict(i=None), -1, -1), (dict(o=None), -1, -1),
        (dict(nz=ENV_MAX_N + 1), -1, -1), (dict(nx=1 << 20, nz=ENV_MAX_N), -1, -1),
        (dict(o="a"), 0, -1),                                                # rf == env: the host form stages them apart
        (dict(nx=0), 0, 0), (dict(nz=0), 0, 0), (dict(nx=0, nz=ENV_MAX_N + 1), -1, -1),
    ],
    log_compress: [
        (dict(), 0, 0), (dict(o="a"), 0, 0),                                 # (in place: no rule against it)
        (dict(i=None), -1, -1), (dict(o=None), -1, -1),
        (dict(dr=0.0), -1, -1), (dict(dr=-50.0), -1, -1), (dict(dr=NAN), -1, -1),
        (dict(n=0), 0, 0), (dict(n=0, dr=0.0), -1, -1),
    ],
    axial_fir: [
        (dict(), 0, 0), (dict(K=0), 0, 0),
        (dict(taps=None), -1, -1), (dict(i=None), -1, -1), (dict(o=None), -1, -1), (dict(o="a"), -1, -1),
        (dict(K=FIR_MAX_K + 1), -1, -1), (dict(nz=0), -1, -1), (dict(nx=0, nz=0), -1, -1),
        (dict(nx=65536, nz=65536), -1, -1), (dict(nx=1 << 31, nz=1), -1, -1),  # 2^32 samples; 2^31 workgroups
        (dict(nx=0), 0, 0),
    ],
    rf2iq: [
        (dict(), 0, 0), (dict(D=1, T=8), 0, 0),
        (dict(taps=None), -1, -1), (dict(i=None), -1, -1), (dict(o=None), -1, -1), (dict(o="a"), -1, -1),
        (dict(T=0), -1, -1), (dict(D=0), -1, -1), (dict(D=RF2IQ_MAX_D + 1), -1, -1), (dict(K=FIR_MAX_K + 1), -1, -1),
        (dict(fs=0.0), -1, -1), (dict(fs=INF), -1, -1), (dict(t0=NAN), -1, -1), (dict(fd=-1.0), -1, -1), (dict(fd=NAN), -1, -1),
        (dict(nt=65536, T=65536), -1, -1), (dict(nt=1 << 31, T=1), -1, -1),
        (dict(nt=0), 0, 0), (dict(nt=0, T=0), -1, -1),
    ],
    iq_envelope: [
        (dict(), 0, 0),
        (dict(i=None), -1, -1), (dict(o=None), -1, -1), (dict(o="a"), -1, -1),
        (dict(n=0), 0, 0), (dict(n=0, i=None), -1, -1),
    ],
    scan_convert: [
        (dict(), 0, 0),
        (dict(null_params=True), -1, -1), (dict(src=None), -1, -1), (dict(x=None), -1, -1), (dict(z=None), -1, -1), (dict(dst=None), -1, -1),
        (dict(n_theta=1), -1, -1), (dict(n_rho=1), -1, -1), (dict(nx=0), -1, -1), (dict(nz=0), -1, -1),
        (dict(n_theta=65536, n_rho=65536), -1, -1), (dict(nx=65536, nz=65536), -1, -1),
        (dict(theta0=NAN), -1, -1), (dict(dtheta=INF), -1, -1), (dict(rho0=-INF), -1, -1), (dict(drho=NAN), -1, -1),
        (dict(ox=INF), -1, -1), (dict(oz=NAN), -1, -1), (dict(dtheta=0.0), -1, -1), (dict(drho=0.0), -1, -1),
        (dict(dst="a"), -1, -1),
    ],
}
ENTRY = {pulse: "pbrt_us_apply_pulse", envelope: "pbrt_envelope", log_compress: "pbrt_log_compress", axial_fir: "pbrt_axial_fir",
         rf2iq: "pbrt_rf2iq", iq_envelope: "pbrt_iq_envelope", scan_convert: "pbrt_scan_convert"}
# an empty call of each step that has one
EMPTY = [(pulse, dict(nt=0)), (pulse, dict(T=0)), (envelope, dict(nx=0)), (envelope, dict(nz=0)), (log_compress, dict(n=0)),
         (axial_fir, dict(nx=0)), (rf2iq, dict(nt=0)), (iq_envelope, dict(n=0))]


def _kw(step, capi, kw):
    return dict(kw, capi=capi) if step is scan_convert else kw


@pytest.mark.parametrize("form", ["host", "dev"])
@pytest.mark.parametrize("step", list(CASES), ids=lambda s: s.__name__)
def test_every_rule_an_accepted_call_and_the_empty_calls(forms, capi, step, form):
    L = forms[form]
    for kw, rc_host, rc_dev in CASES[step]:
        want = rc_dev if L.dev else rc_host
        assert want in (0, -1)
        got = step(L, **_kw(step, capi, kw))
        assert got == want, (step.__name__, form, kw, L.lib.pbrt_last_error(L.ctx.handle))
        if want == -1:
            assert L.lib.pbrt_last_error(L.ctx.handle).decode().startswith("invalid argument: "), (step.__name__, form, kw)
    L.ctx.synchronize()
    # a null context is refused before anything else is looked at: an accepted, a refused and an empty call
    assert step(L, **_kw(step, capi, {}), handle=False) == -1
    assert step(L, **_kw(step, capi, CASES[step][1][0]), handle=False) == -1
    for s, kw in EMPTY:
        if s is step:
            assert step(L, **kw, handle=False) == -1


def test_host_forms_are_refused_while_a_recording_is_open(forms, mi, capi):
    H, D = forms["host"], forms["dev"]
    ctx, lib = H.ctx, H.lib
    assert log_compress(D) == 0                                              # (the buffer of the maxima exists before the recording)
    ctx.synchronize()
    with ctx.record() as rec:
        assert log_compress(D) == 0                                          # a queueing form records
        for step in CASES:
            assert step(H, **_kw(step, capi, {})) == -1, step.__name__
            msg = lib.pbrt_last_error(ctx.handle).decode()
            assert msg.startswith("a recording is open on this context") and msg.endswith(ENTRY[step] + " cannot run"), msg
        for step, kw in EMPTY:                                               # nothing to do: nothing to refuse
            assert step(H, **kw) == 0, (step.__name__, kw)
            assert step(D, **kw) == 0, (step.__name__, kw)
    rec.graph.launch()                                                       # the recording stayed good
    ctx.synchronize()
    rec.graph.close()
    for step in CASES:
        assert step(H, **_kw(step, capi, {})) == 0, step.__name__

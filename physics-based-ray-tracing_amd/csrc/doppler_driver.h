// The driver of the two Doppler steps (include/pbrt_hip.h "colour and power Doppler", DESIGN D24), included by pbrt_api.hip inside its
// extern "C" block, after the image steps whose macros it uses (MAKE_REQUEST, STAGED_BEGIN, STAGED_RUN, IMG_LAUNCH, launched): the two
// launches as their requests shape them (doppler_request.h), and the four entry points.
#pragma once

// the two Doppler steps (doppler_request.h, DESIGN D24): the autocorrelation by the number of wall-filter coefficients, then the maps
static int doppler_acf_enqueue(pbrt_ctx *c, const DopplerAcfRequest &rq, const float *dframes, const float *dq, float *dacf) {
    const float2 *f = reinterpret_cast<const float2 *>(dframes);
    switch (rq.n_coef) {  // (doppler_acf_request admits 0 .. DOPPLER_MAX_DEGREE + 1)
        case 0: IMG_LAUNCH(c, rq.launch, k_doppler_autocorr<0>, rq.N, rq.P, f, dq, dacf); break;
        case 1: IMG_LAUNCH(c, rq.launch, k_doppler_autocorr<1>, rq.N, rq.P, f, dq, dacf); break;
        case 2: IMG_LAUNCH(c, rq.launch, k_doppler_autocorr<2>, rq.N, rq.P, f, dq, dacf); break;
        case 3: IMG_LAUNCH(c, rq.launch, k_doppler_autocorr<3>, rq.N, rq.P, f, dq, dacf); break;
        case 4: IMG_LAUNCH(c, rq.launch, k_doppler_autocorr<4>, rq.N, rq.P, f, dq, dacf); break;
        default: return c->fail(PBRT_E_INVALID, "invalid argument: wall filter of %u coefficients", rq.n_coef);
    }
    return launched(c);
}
static int doppler_maps_enqueue(pbrt_ctx *c, const DopplerMapsRequest &rq, const float *dacf, float *dvel, float *damp) {
    IMG_LAUNCH(c, rq.launch, k_doppler_maps, rq.nx, rq.nz, rq.kx, rq.kz, rq.tiles_z, rq.scale, rq.w, dacf, dvel, damp);
    return launched(c);
}

// The Doppler steps (doppler_request.h): the two sequences of the image steps above, on lines of their own.  A _dev form: null context
// -> request -> refused -> empty -> hipSetDevice, then it queues; a host form stages its arrays (the outputs named first), queues,
// downloads and waits.
int pbrt_doppler_autocorr_dev(pbrt_ctx *ctx, const pbrt_doppler_params *p, const void *d_frames, const void *d_q, void *d_acf) {
    MAKE_REQUEST(ctx, DopplerAcfRequest, doppler_acf_request, p, d_frames, d_q, d_acf);
    if (rq.empty) return PBRT_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return doppler_acf_enqueue(ctx, rq, (const float *)d_frames, (const float *)d_q, (float *)d_acf);
}
int pbrt_doppler_autocorr(pbrt_ctx *ctx, const pbrt_doppler_params *p, const float *frames, const float *q, float *acf) {
    MAKE_REQUEST(ctx, DopplerAcfRequest, doppler_acf_request, p, frames, q, acf);
    STAGED_BEGIN(ctx, rq.empty);
    auto [dacf, df, dq] = S.arrays(stage_out(acf, 3 * (size_t)rq.P), stage_in(frames, 2 * (size_t)rq.N * rq.P),
                                   stage_in(rq.n_coef ? q : nullptr, (size_t)rq.n_coef * rq.N));
    STAGED_RUN(S, doppler_acf_enqueue(ctx, rq, df, dq, dacf));
}
int pbrt_doppler_maps_dev(pbrt_ctx *ctx, const pbrt_doppler_params *p, const void *d_acf, void *d_velocity, void *d_amplitude) {
    MAKE_REQUEST(ctx, DopplerMapsRequest, doppler_maps_request, p, d_acf, d_velocity, d_amplitude);
    if (rq.empty) return PBRT_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return doppler_maps_enqueue(ctx, rq, (const float *)d_acf, (float *)d_velocity, (float *)d_amplitude);
}
int pbrt_doppler_maps(pbrt_ctx *ctx, const pbrt_doppler_params *p, const float *acf, float *velocity, float *amplitude) {
    MAKE_REQUEST(ctx, DopplerMapsRequest, doppler_maps_request, p, acf, velocity, amplitude);
    STAGED_BEGIN(ctx, rq.empty);
    const size_t n = (size_t)rq.nx * rq.nz;
    auto [dvel, damp, dacf] = S.arrays(stage_out(velocity, n), stage_out(amplitude, n), stage_in(acf, 3 * n));
    STAGED_RUN(S, doppler_maps_enqueue(ctx, rq, dacf, dvel, damp));
}

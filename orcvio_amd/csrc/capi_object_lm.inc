// ---- the object optimiser (SURVEY.md 8a row 11): batched Levenberg-Marquardt over object tracks ----------------------------------
// Replaces ObjectFeatureInitializer::single_levenberg_marquardt (src/obj/ObjectFeatureInitializer.cpp:346-440) for every object of
// a frame at once: tracks with a start value in, the optimum out, one launch (k_object_lm, one workgroup per object) and one wait.
// The staging is the call's own (h_lm / d_lm): neither the resident covariance nor the arena of an open io_begin is touched.
void orcvio_msckf_object_lm_config_default(orcvio_object_lm_config* cfg) {
    if (!cfg) return;
    cfg->use_left_perturbation = 1;
    cfg->use_new_bbox_residual = 0;
    for (int i = 0; i < 4; ++i) cfg->residual_weights[i] = 1.0;
    cfg->max_iter = 60;
    cfg->ptol = 1e-18;
}

static int object_lm_reserve(orcvio_msckf_handle* h, size_t bytes) {
    if (bytes <= h->lm_cap) return ORCVIO_OK;
    if (h->h_lm) (void)hipHostFree(h->h_lm);
    if (h->d_lm) (void)hipFree(h->d_lm);
    h->h_lm = nullptr; h->d_lm = nullptr; h->lm_cap = 0;
    const size_t cap = (bytes * 3 / 2 + 4095) & ~(size_t)4095;
    HIPCHK(hipHostMalloc(&h->h_lm, cap, hipHostMallocDefault));
    HIPCHK(hipMalloc(&h->d_lm, cap));
    h->lm_cap = cap;
    return ORCVIO_OK;
}

int32_t orcvio_msckf_object_lm(orcvio_msckf_handle* h, const orcvio_object_lm_config* cfg, const orcvio_object_track* tracks,
                               const orcvio_object_lm_prior* priors, int32_t n_tracks, orcvio_object_lm_result* results) {
    if (!h) { g_last_error = "object_lm: null handle"; return ORCVIO_ERR_INVALID; }
    const char* why = "";
    size_t nd = 0;
    const int rv = obj_lm_validate(cfg, tracks, priors, n_tracks, results, h->maxF, &why, &nd);
    if (rv != ORCVIO_OK) { g_last_error = std::string("object_lm: ") + why; return rv; }
    if (n_tracks == 0) return ORCVIO_OK;
    HIPCHK(hipSetDevice(h->device));
    // [records | inputs | outputs], 16-byte records in front of the doubles
    const size_t o_in = sizeof(ObjLmTrack) * (size_t)n_tracks, o_out = o_in + nd * sizeof(double);
    const size_t total = o_out + sizeof(double) * OBJ_LM_OUT * (size_t)n_tracks;
    int rc;
    if ((rc = object_lm_reserve(h, total)) != ORCVIO_OK) return rc;
    obj_lm_pack(tracks, priors, n_tracks, reinterpret_cast<ObjLmTrack*>(h->h_lm), reinterpret_cast<double*>(h->h_lm + o_in));
    hipStream_t s = h->stream;
    HIPCHK(hipMemcpyAsync(h->d_lm, h->h_lm, o_out, hipMemcpyHostToDevice, s));
    ObjLmArgs a;
    a.tracks = reinterpret_cast<const ObjLmTrack*>(h->d_lm);
    a.in = reinterpret_cast<const double*>(h->d_lm + o_in);
    a.out = reinterpret_cast<double*>(h->d_lm + o_out);
    a.obj_left = cfg->use_left_perturbation ? 1 : 0;
    a.new_bbox = cfg->use_new_bbox_residual;
    a.max_iter = cfg->max_iter;
    for (int i = 0; i < 4; ++i) a.w[i] = cfg->residual_weights[i];
    a.ptol = cfg->ptol;
    hipLaunchKernelGGL(k_object_lm, dim3(n_tracks), dim3(OBJ_LM_NT), 0, s, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h->h_lm + o_out, h->d_lm + o_out, total - o_out, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    obj_lm_unpack(reinterpret_cast<const double*>(h->h_lm + o_out), tracks, n_tracks, results);
    return ORCVIO_OK;
}

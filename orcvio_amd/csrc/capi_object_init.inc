// ---- the start of an object track: keypoint triangulation and Kabsch alignment on the device ------------------------------------
// Replaces ObjectFeatureInitializer::single_object_initialization (src/obj/ObjectFeatureInitializer.cpp:33-198) for every object of
// a frame at once (k_object_init, one workgroup per object), alone or in front of the optimiser in the same call.  The staging is
// the optimiser's (h_lm / d_lm, object_lm_reserve): [records | inputs | initialiser's outputs | optimiser's outputs].
void orcvio_msckf_object_init_config_default(orcvio_object_init_config* cfg) {
    if (!cfg) return;
    cfg->pose_form = 1;
    cfg->min_obs = 3;
    cfg->min_kps = 3;
}

// both entry points behind their validation: lm_cfg == nullptr is the initialiser alone
static int32_t object_init_run(orcvio_msckf_handle* h, const orcvio_object_init_config* cfg, const orcvio_object_lm_config* lm_cfg,
                               const orcvio_object_track* tracks, const double* const* mean_kps_per_track, const orcvio_object_lm_prior* priors,
                               int32_t n_tracks, size_t nd, orcvio_object_init_result* results, orcvio_object_lm_result* lm_results) {
    HIPCHK(hipSetDevice(h->device));
    const size_t o_in = sizeof(ObjLmTrack) * (size_t)n_tracks, o_out = o_in + nd * sizeof(double);
    const size_t o_lm = o_out + sizeof(double) * OBJ_INIT_OUT * (size_t)n_tracks;
    const size_t total = o_lm + (lm_cfg ? sizeof(double) * OBJ_LM_OUT * (size_t)n_tracks : 0);
    int rc;
    if ((rc = object_lm_reserve(h, total)) != ORCVIO_OK) return rc;
    obj_init_pack(tracks, mean_kps_per_track, priors, n_tracks, reinterpret_cast<ObjLmTrack*>(h->h_lm), reinterpret_cast<double*>(h->h_lm + o_in));
    hipStream_t s = h->stream;
    HIPCHK(hipMemcpyAsync(h->d_lm, h->h_lm, o_out, hipMemcpyHostToDevice, s));
    ObjInitArgs ia;
    ia.tracks = reinterpret_cast<ObjLmTrack*>(h->d_lm);
    ia.in = reinterpret_cast<double*>(h->d_lm + o_in);
    ia.out = reinterpret_cast<double*>(h->d_lm + o_out);
    ia.pose_form = cfg->pose_form; ia.min_obs = cfg->min_obs; ia.min_kps = cfg->min_kps;
    hipLaunchKernelGGL(k_object_init, dim3(n_tracks), dim3(OBJ_INIT_NT), 0, s, ia);
    HIPCHK(hipGetLastError());
    if (lm_cfg) {
        ObjLmArgs a;
        a.tracks = ia.tracks;
        a.in = ia.in;
        a.out = reinterpret_cast<double*>(h->d_lm + o_lm);
        a.obj_left = lm_cfg->use_left_perturbation ? 1 : 0;
        a.new_bbox = lm_cfg->use_new_bbox_residual;
        a.max_iter = lm_cfg->max_iter;
        for (int i = 0; i < 4; ++i) a.w[i] = lm_cfg->residual_weights[i];
        a.ptol = lm_cfg->ptol;
        hipLaunchKernelGGL(k_object_lm, dim3(n_tracks), dim3(OBJ_LM_NT), 0, s, a);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(h->h_lm + o_out, h->d_lm + o_out, total - o_out, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    obj_init_unpack(reinterpret_cast<const double*>(h->h_lm + o_out), tracks, n_tracks, results);
    if (lm_cfg) obj_lm_unpack(reinterpret_cast<const double*>(h->h_lm + o_lm), tracks, n_tracks, lm_results);
    return ORCVIO_OK;
}

int32_t orcvio_msckf_object_init(orcvio_msckf_handle* h, const orcvio_object_init_config* cfg, const orcvio_object_track* tracks,
                                 const double* const* mean_kps_per_track, int32_t n_tracks, orcvio_object_init_result* results) {
    if (!h) { g_last_error = "object_init: null handle"; return ORCVIO_ERR_INVALID; }
    const char* why = "";
    size_t nd = 0;
    const int rv = obj_init_validate(cfg, tracks, mean_kps_per_track, n_tracks, results, h->maxF, &why, &nd);
    if (rv != ORCVIO_OK) { g_last_error = std::string("object_init: ") + why; return rv; }
    if (n_tracks == 0) return ORCVIO_OK;
    return object_init_run(h, cfg, nullptr, tracks, mean_kps_per_track, nullptr, n_tracks, nd, results, nullptr);
}

int32_t orcvio_msckf_object_init_lm(orcvio_msckf_handle* h, const orcvio_object_init_config* init_cfg, const orcvio_object_lm_config* lm_cfg,
                                    const orcvio_object_track* tracks, const orcvio_object_lm_prior* priors, int32_t n_tracks,
                                    orcvio_object_init_result* init_results, orcvio_object_lm_result* lm_results) {
    if (!h) { g_last_error = "object_init_lm: null handle"; return ORCVIO_ERR_INVALID; }
    const char* why = "";
    size_t nd = 0;
    const int rv = obj_init_lm_validate(init_cfg, lm_cfg, tracks, priors, n_tracks, init_results, lm_results, h->maxF, &why, &nd);
    if (rv != ORCVIO_OK) { g_last_error = std::string("object_init_lm: ") + why; return rv; }
    if (n_tracks == 0) return ORCVIO_OK;
    return object_init_run(h, init_cfg, lm_cfg, tracks, nullptr, priors, n_tracks, nd, init_results, lm_results);
}

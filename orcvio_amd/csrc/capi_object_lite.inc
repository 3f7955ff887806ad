// ---- the lite (bbox-only) object mapper: the start from the first bounding box and the 9-dof Levenberg-Marquardt ------------------
// Replaces ObjectFeatureInitializer::single_object_initialization_lite (src/obj/ObjectFeatureInitializer.cpp:495-584) and
// single_levenberg_marquardt_lite (:442-493) for every object of a frame at once: k_object_init_lite (one thread per object) and
// k_object_lm_lite (one wavefront per object), alone or one behind the other in the same call.  The staging is the optimiser's
// (h_lm / d_lm, object_lm_reserve): [records | inputs | initialiser's outputs | optimiser's outputs].
void orcvio_msckf_object_lite_config_default(orcvio_object_lite_config* cfg) {
    if (!cfg) return;
    cfg->use_left_perturbation = 1;
    cfg->use_new_bbox_residual = 0;
    cfg->residual_weights[0] = cfg->residual_weights[1] = 1.0;
    cfg->reg_every_frame = 0;
    cfg->max_iter = 60;
    cfg->ptol = 1e-18;
}

void orcvio_msckf_object_init_lite_config_default(orcvio_object_init_lite_config* cfg) {
    if (!cfg) return;
    cfg->pose_form = 1;
    cfg->bbox_scale[0] = cfg->bbox_scale[1] = cfg->bbox_scale[2] = 1.0;
}

// the three entry points behind their validation: init_cfg == nullptr is the optimiser alone, lm_cfg == nullptr the initialiser alone
// (the mean shapes come from `priors`, or from `means` where there are no priors)
static int32_t object_lite_run(orcvio_msckf_handle* h, const orcvio_object_init_lite_config* init_cfg, const orcvio_object_lite_config* lm_cfg,
                               const orcvio_object_track* tracks, const orcvio_object_lm_prior* priors, const double* const* means,
                               int32_t n_tracks, size_t nd, orcvio_object_init_lite_result* init_results, orcvio_object_lm_result* lm_results) {
    auto mean = [&](int q) { return priors ? priors[q].mean_shape : means[q]; };
    HIPCHK(hipSetDevice(h->device));
    const size_t o_in = sizeof(ObjLmTrack) * (size_t)n_tracks, o_out = o_in + nd * sizeof(double);
    const size_t o_lm = o_out + (init_cfg ? sizeof(double) * OBJ_LITE_INIT_OUT * (size_t)n_tracks : 0);
    const size_t total = o_lm + (lm_cfg ? sizeof(double) * OBJ_LITE_OUT * (size_t)n_tracks : 0);
    int rc;
    if ((rc = object_lm_reserve(h, total)) != ORCVIO_OK) return rc;
    obj_lite_pack(tracks, mean, n_tracks, init_cfg == nullptr, reinterpret_cast<ObjLmTrack*>(h->h_lm), reinterpret_cast<double*>(h->h_lm + o_in));
    hipStream_t s = h->stream;
    HIPCHK(hipMemcpyAsync(h->d_lm, h->h_lm, o_out, hipMemcpyHostToDevice, s));
    if (init_cfg) {
        ObjLiteInitArgs ia;
        ia.tracks = reinterpret_cast<ObjLmTrack*>(h->d_lm);
        ia.in = reinterpret_cast<double*>(h->d_lm + o_in);
        ia.out = reinterpret_cast<double*>(h->d_lm + o_out);
        ia.n_tracks = n_tracks;
        ia.pose_form = init_cfg->pose_form;
        for (int i = 0; i < 3; ++i) ia.bbox_scale[i] = init_cfg->bbox_scale[i];
        hipLaunchKernelGGL(k_object_init_lite, dim3((n_tracks + 63) / 64), dim3(64), 0, s, ia);
        HIPCHK(hipGetLastError());
    }
    if (lm_cfg) {
        ObjLiteArgs a;
        a.tracks = reinterpret_cast<const ObjLmTrack*>(h->d_lm);
        a.in = reinterpret_cast<const double*>(h->d_lm + o_in);
        a.out = reinterpret_cast<double*>(h->d_lm + o_lm);
        a.n_tracks = n_tracks;
        a.obj_left = lm_cfg->use_left_perturbation ? 1 : 0;
        a.new_bbox = lm_cfg->use_new_bbox_residual;
        a.reg_every_frame = lm_cfg->reg_every_frame ? 1 : 0;
        a.max_iter = lm_cfg->max_iter;
        a.w[0] = lm_cfg->residual_weights[0]; a.w[1] = lm_cfg->residual_weights[1];
        a.ptol = lm_cfg->ptol;
        hipLaunchKernelGGL(k_object_lm_lite, dim3((n_tracks + OBJ_LITE_WPB - 1) / OBJ_LITE_WPB), dim3(OBJ_LITE_NT), 0, s, a);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(h->h_lm + o_out, h->d_lm + o_out, total - o_out, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (init_cfg) obj_lite_init_unpack(reinterpret_cast<const double*>(h->h_lm + o_out), n_tracks, init_results);
    if (lm_cfg) obj_lite_unpack(reinterpret_cast<const double*>(h->h_lm + o_lm), n_tracks, lm_results);
    return ORCVIO_OK;
}

int32_t orcvio_msckf_object_lm_lite(orcvio_msckf_handle* h, const orcvio_object_lite_config* cfg, const orcvio_object_track* tracks,
                                    const orcvio_object_lm_prior* priors, int32_t n_tracks, orcvio_object_lm_result* results) {
    if (!h) { g_last_error = "object_lm_lite: null handle"; return ORCVIO_ERR_INVALID; }
    const char* why = "";
    size_t nd = 0;
    const int rv = obj_lite_lm_validate(cfg, tracks, priors, n_tracks, results, h->maxF, &why, &nd);
    if (rv != ORCVIO_OK) { g_last_error = std::string("object_lm_lite: ") + why; return rv; }
    if (n_tracks == 0) return ORCVIO_OK;
    return object_lite_run(h, nullptr, cfg, tracks, priors, nullptr, n_tracks, nd, nullptr, results);
}

int32_t orcvio_msckf_object_init_lite(orcvio_msckf_handle* h, const orcvio_object_init_lite_config* cfg, const orcvio_object_track* tracks,
                                      const double* const* mean_shape_per_track, int32_t n_tracks, orcvio_object_init_lite_result* results) {
    if (!h) { g_last_error = "object_init_lite: null handle"; return ORCVIO_ERR_INVALID; }
    const char* why = "";
    size_t nd = 0;
    const int rv = obj_lite_init_validate(cfg, tracks, mean_shape_per_track, n_tracks, results, h->maxF, &why, &nd);
    if (rv != ORCVIO_OK) { g_last_error = std::string("object_init_lite: ") + why; return rv; }
    if (n_tracks == 0) return ORCVIO_OK;
    return object_lite_run(h, cfg, nullptr, tracks, nullptr, mean_shape_per_track, n_tracks, nd, results, nullptr);
}

int32_t orcvio_msckf_object_init_lm_lite(orcvio_msckf_handle* h, const orcvio_object_init_lite_config* init_cfg,
                                         const orcvio_object_lite_config* lm_cfg, const orcvio_object_track* tracks,
                                         const orcvio_object_lm_prior* priors, int32_t n_tracks,
                                         orcvio_object_init_lite_result* init_results, orcvio_object_lm_result* lm_results) {
    if (!h) { g_last_error = "object_init_lm_lite: null handle"; return ORCVIO_ERR_INVALID; }
    const char* why = "";
    size_t nd = 0;
    const int rv = obj_lite_init_lm_validate(init_cfg, lm_cfg, tracks, priors, n_tracks, init_results, lm_results, h->maxF, &why, &nd);
    if (rv != ORCVIO_OK) { g_last_error = std::string("object_init_lm_lite: ") + why; return rv; }
    if (n_tracks == 0) return ORCVIO_OK;
    return object_lite_run(h, init_cfg, lm_cfg, tracks, priors, nullptr, n_tracks, nd, init_results, lm_results);
}

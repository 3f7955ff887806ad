// ---- the object mapper (SURVEY.md 8a row 11): the start and the Levenberg-Marquardt refinement of object tracks, batched -------------
// Replaces, for every object of a frame at once, ObjectFeatureInitializer's (src/obj/ObjectFeatureInitializer.cpp)
//   single_levenberg_marquardt (:346-440)           orcvio_msckf_object_lm        k_object_lm, one workgroup per object
//   single_object_initialization (:33-198)          orcvio_msckf_object_init      k_object_init, one workgroup per object
//   single_levenberg_marquardt_lite (:442-493)      orcvio_msckf_object_lm_lite   k_object_lm_lite, one wavefront per object
//   single_object_initialization_lite (:495-584)    orcvio_msckf_object_init_lite k_object_init_lite, one thread per object
// and the two _init_lm calls: the initialiser with the optimiser behind it on the same staged block, one wait.
// The staging is the calls' own (h_lm / d_lm): neither the resident covariance nor the arena of an open io_begin is touched.
void orcvio_msckf_object_lm_config_default(orcvio_object_lm_config* cfg) {
    if (!cfg) return;
    cfg->use_left_perturbation = 1;
    cfg->use_new_bbox_residual = 0;
    for (int i = 0; i < 4; ++i) cfg->residual_weights[i] = 1.0;
    cfg->max_iter = 60;
    cfg->ptol = 1e-18;
}

void orcvio_msckf_object_init_config_default(orcvio_object_init_config* cfg) {
    if (!cfg) return;
    cfg->pose_form = 1;
    cfg->min_obs = 3;
    cfg->min_kps = 3;
}

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

extern "C++" {   // (overloads and a template: not for the C linkage this file is included under)
// one launch per config type: the kernel's arguments are filled from the config here and nowhere else
static void object_launch(const orcvio_object_init_config& c, ObjLmTrack* recs, double* in, double* out, int n_tracks, hipStream_t s) {
    ObjInitArgs a;
    a.tracks = recs; a.in = in; a.out = out;
    a.pose_form = c.pose_form; a.min_obs = c.min_obs; a.min_kps = c.min_kps;
    hipLaunchKernelGGL(k_object_init, dim3(n_tracks), dim3(OBJ_INIT_NT), 0, s, a);
}
static void object_launch(const orcvio_object_lm_config& c, ObjLmTrack* recs, double* in, double* out, int n_tracks, hipStream_t s) {
    ObjLmArgs a;
    a.tracks = recs; a.in = in; a.out = out;
    a.obj_left = c.use_left_perturbation ? 1 : 0;
    a.new_bbox = c.use_new_bbox_residual;
    a.max_iter = c.max_iter;
    for (int i = 0; i < 4; ++i) a.w[i] = c.residual_weights[i];
    a.ptol = c.ptol;
    hipLaunchKernelGGL(k_object_lm, dim3(n_tracks), dim3(OBJ_LM_NT), 0, s, a);
}
static void object_launch(const orcvio_object_init_lite_config& c, ObjLmTrack* recs, double* in, double* out, int n_tracks, hipStream_t s) {
    ObjLiteInitArgs a;
    a.tracks = recs; a.in = in; a.out = out;
    a.n_tracks = n_tracks;
    a.pose_form = c.pose_form;
    for (int i = 0; i < 3; ++i) a.bbox_scale[i] = c.bbox_scale[i];
    hipLaunchKernelGGL(k_object_init_lite, dim3((n_tracks + 63) / 64), dim3(64), 0, s, a);
}
static void object_launch(const orcvio_object_lite_config& c, ObjLmTrack* recs, double* in, double* out, int n_tracks, hipStream_t s) {
    ObjLiteArgs a;
    a.tracks = recs; a.in = in; a.out = out;
    a.n_tracks = n_tracks;
    a.obj_left = c.use_left_perturbation ? 1 : 0;
    a.new_bbox = c.use_new_bbox_residual;
    a.reg_every_frame = c.reg_every_frame ? 1 : 0;
    a.max_iter = c.max_iter;
    a.w[0] = c.residual_weights[0]; a.w[1] = c.residual_weights[1];
    a.ptol = c.ptol;
    hipLaunchKernelGGL(k_object_lm_lite, dim3((n_tracks + OBJ_LITE_WPB - 1) / OBJ_LITE_WPB), dim3(OBJ_LITE_NT), 0, s, a);
}

// Every entry point behind its validation (n_tracks > 0): [records | inputs | initialiser's outputs | optimiser's outputs], 16-byte
// records in front of the doubles; one copy in, the initialiser's launch (init_cfg != nullptr), the optimiser's (lm_cfg != nullptr),
// one copy out, one wait.  `io` says what is staged; `res` has the caller's result records of the launches that run.
struct ObjMapResults {
    orcvio_object_init_result* init = nullptr;
    orcvio_object_init_lite_result* init_lite = nullptr;
    orcvio_object_lm_result* lm = nullptr;
};
template <class InitCfg, class LmCfg>
static int32_t object_mapper_run(orcvio_msckf_handle* h, const ObjMapIo& io, const InitCfg* init_cfg, const LmCfg* lm_cfg,
                                 const orcvio_object_track* tracks, int32_t n_tracks, size_t nd, const ObjMapResults res) {
    HIPCHK(hipSetDevice(h->device));
    const size_t init_out = !init_cfg ? 0 : (io.keypoints ? OBJ_INIT_OUT : OBJ_LITE_INIT_OUT);
    const size_t lm_out = !lm_cfg ? 0 : (io.keypoints ? OBJ_LM_OUT : OBJ_LITE_OUT);
    const size_t o_in = sizeof(ObjLmTrack) * (size_t)n_tracks, o_out = o_in + nd * sizeof(double);
    const size_t o_lm = o_out + sizeof(double) * init_out * (size_t)n_tracks;
    const size_t total = o_lm + sizeof(double) * lm_out * (size_t)n_tracks;
    int rc;
    if ((rc = object_lm_reserve(h, total)) != ORCVIO_OK) return rc;
    obj_map_pack(io, tracks, n_tracks, reinterpret_cast<ObjLmTrack*>(h->h_lm), reinterpret_cast<double*>(h->h_lm + o_in));
    hipStream_t s = h->stream;
    HIPCHK(hipMemcpyAsync(h->d_lm, h->h_lm, o_out, hipMemcpyHostToDevice, s));
    ObjLmTrack* recs = reinterpret_cast<ObjLmTrack*>(h->d_lm);
    double* in = reinterpret_cast<double*>(h->d_lm + o_in);
    if (init_cfg) {
        object_launch(*init_cfg, recs, in, reinterpret_cast<double*>(h->d_lm + o_out), n_tracks, s);
        HIPCHK(hipGetLastError());
    }
    if (lm_cfg) {
        object_launch(*lm_cfg, recs, in, reinterpret_cast<double*>(h->d_lm + o_lm), n_tracks, s);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(h->h_lm + o_out, h->d_lm + o_out, total - o_out, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const double* r_init = reinterpret_cast<const double*>(h->h_lm + o_out);
    const double* r_lm = reinterpret_cast<const double*>(h->h_lm + o_lm);
    if (init_cfg && io.keypoints) obj_init_unpack(r_init, tracks, n_tracks, res.init);
    if (init_cfg && !io.keypoints) obj_lite_init_unpack(r_init, n_tracks, res.init_lite);
    if (lm_cfg && io.keypoints) obj_lm_unpack(r_lm, tracks, n_tracks, res.lm);
    if (lm_cfg && !io.keypoints) obj_lite_unpack(r_lm, n_tracks, res.lm);
    return ORCVIO_OK;
}

}  // extern "C++"

// what an entry point returns without a launch: the null handle, the validator's refusal under the entry point's name, or no tracks
static int32_t object_mapper_verdict(const char* name, const orcvio_msckf_handle* h, int rv, const char* why) {
    if (!h) { g_last_error = std::string(name) + ": null handle"; return ORCVIO_ERR_INVALID; }
    if (rv != ORCVIO_OK) g_last_error = std::string(name) + ": " + why;
    return rv;
}

int32_t orcvio_msckf_object_lm(orcvio_msckf_handle* h, const orcvio_object_lm_config* cfg, const orcvio_object_track* tracks,
                               const orcvio_object_lm_prior* priors, int32_t n_tracks, orcvio_object_lm_result* results) {
    const char* why = "";
    size_t nd = 0;
    const int rv = h ? obj_lm_validate(cfg, tracks, priors, n_tracks, results, h->maxF, &why, &nd) : ORCVIO_ERR_INVALID;
    if (rv != ORCVIO_OK || n_tracks == 0) return object_mapper_verdict("object_lm", h, rv, why);
    return object_mapper_run<orcvio_object_init_config>(h, obj_io_lm(priors, results), nullptr, cfg, tracks, n_tracks, nd, {nullptr, nullptr, results});
}

int32_t orcvio_msckf_object_init(orcvio_msckf_handle* h, const orcvio_object_init_config* cfg, const orcvio_object_track* tracks,
                                 const double* const* mean_kps_per_track, int32_t n_tracks, orcvio_object_init_result* results) {
    const char* why = "";
    size_t nd = 0;
    const int rv = h ? obj_init_validate(cfg, tracks, mean_kps_per_track, n_tracks, results, h->maxF, &why, &nd) : ORCVIO_ERR_INVALID;
    if (rv != ORCVIO_OK || n_tracks == 0) return object_mapper_verdict("object_init", h, rv, why);
    return object_mapper_run<orcvio_object_init_config, orcvio_object_lm_config>(h, obj_io_init(mean_kps_per_track, nullptr, results, nullptr), cfg, nullptr,
                                                                                 tracks, n_tracks, nd, {results, nullptr, nullptr});
}

int32_t orcvio_msckf_object_init_lm(orcvio_msckf_handle* h, const orcvio_object_init_config* init_cfg, const orcvio_object_lm_config* lm_cfg,
                                    const orcvio_object_track* tracks, const orcvio_object_lm_prior* priors, int32_t n_tracks,
                                    orcvio_object_init_result* init_results, orcvio_object_lm_result* lm_results) {
    const char* why = "";
    size_t nd = 0;
    const int rv = h ? obj_init_lm_validate(init_cfg, lm_cfg, tracks, priors, n_tracks, init_results, lm_results, h->maxF, &why, &nd) : ORCVIO_ERR_INVALID;
    if (rv != ORCVIO_OK || n_tracks == 0) return object_mapper_verdict("object_init_lm", h, rv, why);
    return object_mapper_run(h, obj_io_init(nullptr, priors, init_results, lm_results), init_cfg, lm_cfg, tracks, n_tracks, nd, {init_results, nullptr, lm_results});
}

int32_t orcvio_msckf_object_lm_lite(orcvio_msckf_handle* h, const orcvio_object_lite_config* cfg, const orcvio_object_track* tracks,
                                    const orcvio_object_lm_prior* priors, int32_t n_tracks, orcvio_object_lm_result* results) {
    const char* why = "";
    size_t nd = 0;
    const int rv = h ? obj_lite_lm_validate(cfg, tracks, priors, n_tracks, results, h->maxF, &why, &nd) : ORCVIO_ERR_INVALID;
    if (rv != ORCVIO_OK || n_tracks == 0) return object_mapper_verdict("object_lm_lite", h, rv, why);
    return object_mapper_run<orcvio_object_init_lite_config>(h, obj_io_lite(priors, nullptr, nullptr, results), nullptr, cfg, tracks, n_tracks, nd,
                                                             {nullptr, nullptr, results});
}

int32_t orcvio_msckf_object_init_lite(orcvio_msckf_handle* h, const orcvio_object_init_lite_config* cfg, const orcvio_object_track* tracks,
                                      const double* const* mean_shape_per_track, int32_t n_tracks, orcvio_object_init_lite_result* results) {
    const char* why = "";
    size_t nd = 0;
    const int rv = h ? obj_lite_init_validate(cfg, tracks, mean_shape_per_track, n_tracks, results, h->maxF, &why, &nd) : ORCVIO_ERR_INVALID;
    if (rv != ORCVIO_OK || n_tracks == 0) return object_mapper_verdict("object_init_lite", h, rv, why);
    return object_mapper_run<orcvio_object_init_lite_config, orcvio_object_lite_config>(h, obj_io_lite(nullptr, mean_shape_per_track, results, nullptr), cfg,
                                                                                        nullptr, tracks, n_tracks, nd, {nullptr, results, nullptr});
}

int32_t orcvio_msckf_object_init_lm_lite(orcvio_msckf_handle* h, const orcvio_object_init_lite_config* init_cfg,
                                         const orcvio_object_lite_config* lm_cfg, const orcvio_object_track* tracks,
                                         const orcvio_object_lm_prior* priors, int32_t n_tracks,
                                         orcvio_object_init_lite_result* init_results, orcvio_object_lm_result* lm_results) {
    const char* why = "";
    size_t nd = 0;
    const int rv = h ? obj_lite_init_lm_validate(init_cfg, lm_cfg, tracks, priors, n_tracks, init_results, lm_results, h->maxF, &why, &nd) : ORCVIO_ERR_INVALID;
    if (rv != ORCVIO_OK || n_tracks == 0) return object_mapper_verdict("object_init_lm_lite", h, rv, why);
    return object_mapper_run(h, obj_io_lite(priors, nullptr, init_results, lm_results), init_cfg, lm_cfg, tracks, n_tracks, nd, {nullptr, init_results, lm_results});
}

// jxl-hip: streaming decode pipeline of one GPU (pipeline.h).  Threads: `prepare_threads` workers (parse, tables, upload), one LF issuer (LF stages in submission
// order, jobs that are ready together as one launch), one issuer (HF stages and tails in submission order); Submit / Wait are called by anybody.  All GPU work goes to non-blocking streams of the object's own; nothing touches the NULL stream.
#include "pipeline.h"
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace jxlhip {

#define HIP_CHECK(expr)                                                                                    \
  do {                                                                                                     \
    hipError_t e_ = (expr);                                                                                \
    if (e_ != hipSuccess) throw ParseError(std::string("HIP error: ") + hipGetErrorString(e_) + " in " #expr, false); \
  } while (0)

namespace {
void* NewStream(int priority) {
  hipStream_t s = nullptr;
  HIP_CHECK(hipStreamCreateWithPriority(&s, hipStreamNonBlocking, priority));
  return s;
}
void* NewEvent(bool timing = false) {
  hipEvent_t e = nullptr;
  HIP_CHECK(hipEventCreateWithFlags(&e, timing ? hipEventDefault : hipEventDisableTiming));
  return e;
}
void Record(void* ev, void* stream) { HIP_CHECK(hipEventRecord((hipEvent_t)ev, (hipStream_t)stream)); }
void StreamWait(void* stream, void* ev) { HIP_CHECK(hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)ev, 0)); }
size_t Align256(size_t v) { return (v + 255) / 256 * 256; }
}  // namespace

// The caller's current device comes back at the end of every public entry point (a thread that drives pipelines on several GPUs, or mixes its own HIP code
// with the pipeline, must not find its device changed after a Submit or a Wait).  The pipeline's own threads stay on their device.
namespace {
struct DeviceScope {
  int prev = -1;
  explicit DeviceScope(int device) { if (hipGetDevice(&prev) != hipSuccess) prev = -1; if (prev != device) (void)hipSetDevice(device); else prev = -1; }
  ~DeviceScope() { if (prev >= 0) (void)hipSetDevice(prev); }
};
}  // namespace

Pipeline::Pipeline(int device, const PipelineOptions& opt) : device_(device), opt_(opt) {
  DeviceScope scope(device_);
  opt_.in_flight = std::max(1, std::min(opt_.in_flight, 64));
  opt_.hf_streams = std::max(1, std::min(opt_.hf_streams, 12));
  opt_.lf_streams = std::max(1, std::min(opt_.lf_streams, 32));
  opt_.prepare_threads = std::max(1, std::min(opt_.prepare_threads, 16));
  opt_.parse_threads = std::max(1, std::min(opt_.parse_threads, 64));
  ncoef_ = opt_.hf_streams + 1;                  // one coefficient set per HF stage in flight + the one the tail is consuming
  // batch objects: the jobs in flight on the GPU + the ones the prepare threads are filling (+ one: a worker waits for its slot's previous job to leave the GPU)
  nbuf_ = opt_.in_flight + 2 + 1;
  if (nbuf_ % ncoef_) nbuf_ += ncoef_ - nbuf_ % ncoef_;     // (job k always meets coefficient set k % ncoef and slot k % nbuf)
  // the few long wavefronts of the entropy stages on high-priority streams, everything else at the default priority (0; the range's other end would be "low")
  int prio_least = 0, prio_high = 0;
  (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_high);   // (numerically lower = higher priority)
  prio_high = std::min(prio_high, 0);
  prio_high_ = prio_high;
  main_ = NewStream(0);
  d2h_[0] = NewStream(0); d2h_[1] = NewStream(0);
  upload_ = NewStream(0);      // (high priority, among the entropy streams' queues, measured the same: profiles/r08_notes.md)
  // LF streams: as many as the hardware queues leave room for (streams that share a queue serialise: eleven LF streams over four queues ran four LF launches at a time
  // and held up the HF stages queued behind them).  JXL_HIP_LF_GROUP_MAX / JXL_HIP_LF_STREAMS_EFFECTIVE: the two options for A/B runs; at creation the environment
  // takes precedence over the options structure, SetOption afterwards over both
  if (const char* e = getenv("JXL_HIP_LF_GROUP_MAX")) opt_.lf_group_max = atoi(e);
  if (const char* e = getenv("JXL_HIP_LF_STREAMS_EFFECTIVE")) opt_.lf_streams_effective = atoi(e);
  lf_group_max_ = std::max(1, std::min(opt_.lf_group_max, kLfGroupMax));
  lf_streams_effective_ = std::max(0, std::min(opt_.lf_streams_effective, opt_.lf_streams));
  lf_side_.reserve(32); lf_side_done_.reserve(32);      // (they grow under mu_ and never move)
  for (int i = 0, n = LfStreamsInUse(); i < n; i++) { lf_side_.push_back(NewStream(prio_high)); lf_side_done_.push_back(nullptr); }
  for (int i = 0; i < opt_.hf_streams; i++) hf_side_.push_back(NewStream(prio_high));
  clock_event_ = NewEvent(true);
  Record(clock_event_, main_);
  coef_.assign((size_t)ncoef_, SharedPlanes());
  for (int b = 0; b < nbuf_; b++) {
    std::unique_ptr<Slot> s(new Slot());
    s->batch.reset(new Batch(device_));
    s->uploaded = NewEvent(); s->lf_done = NewEvent(); s->front_done = NewEvent(); s->hf_done = NewEvent(); s->idct_done = NewEvent(); s->rest_done = NewEvent();
    slots_.push_back(std::move(s));
  }
  if (opt_.reserve_frames > 0 && opt_.reserve_width > 0 && opt_.reserve_height > 0) {
    // layout of Batch::Prepare for plain VarDCT frames: per frame and channel num_groups x 65536 int32 coefficients, one padded float plane
    const size_t ng = (size_t)((opt_.reserve_width + 255) / 256) * ((opt_.reserve_height + 255) / 256);
    const size_t bw = (size_t)(opt_.reserve_width + 7) / 8, bh = (size_t)(opt_.reserve_height + 7) / 8;
    want_coef_ = (size_t)opt_.reserve_frames * 3 * ng * 65536 * 4;
    want_big_ = (size_t)opt_.reserve_frames * 3 * Align256(bw * 8 * bh * 8 * 4) * (size_t)std::max(1, std::min(opt_.reserve_plane_sets, 2));
    ReservePlanes(&big_, want_big_);
    for (auto& c : coef_) ReservePlanes(&c, want_coef_);
  }
  for (int w = 0; w < opt_.prepare_threads; w++) workers_.emplace_back([this, w] { PrepareWorker(w); });
  lf_issuer_ = std::thread([this] { LfIssuerLoop(); });
  issuer_ = std::thread([this] { IssuerLoop(); });
}

int Pipeline::LfStreamsInUse() const {
  const int v = lf_streams_effective_.load();
  return v > 0 ? std::min(v, opt_.lf_streams) : LfStreamsForQueues(opt_.lf_streams, opt_.hf_streams, getenv("GPU_MAX_HW_QUEUES"));
}

bool Pipeline::SetOption(const std::string& name, int value) {
  if (name == "jpeg_region") SetJpegRegion(value != 0);
  else if (name == "lf_group_max") lf_group_max_ = std::max(1, std::min(value, kLfGroupMax));
  else if (name == "lf_streams_effective") lf_streams_effective_ = std::max(0, std::min(value, opt_.lf_streams));
  else return false;
  return true;
}

Pipeline::~Pipeline() {
  { std::lock_guard<std::mutex> lock(mu_); shutdown_ = true; }
  cv_.notify_all();
  for (auto& t : workers_) t.join();
  if (lf_issuer_.joinable()) lf_issuer_.join();
  if (issuer_.joinable()) issuer_.join();
  if (getenv("JXL_HIP_SCHED_TRACE"))
    fprintf(stderr, "[pipe] LF launches since the clock was reset: %lld for %lld jobs, largest group %lld, %d LF streams in use\n", (long long)lf_groups_, (long long)lf_grouped_jobs_, (long long)lf_group_largest_, LfStreamsInUse());
  DeviceScope scope(device_);
  (void)hipStreamSynchronize((hipStream_t)upload_);
  for (void* s : lf_side_) (void)hipStreamSynchronize((hipStream_t)s);
  for (void* s : hf_side_) (void)hipStreamSynchronize((hipStream_t)s);
  (void)hipStreamSynchronize((hipStream_t)main_);
  for (void* s : d2h_) (void)hipStreamSynchronize((hipStream_t)s);
  for (auto& kv : jobs_) if (kv.second->done_event) (void)hipEventDestroy((hipEvent_t)kv.second->done_event);
  jobs_.clear();
  for (auto& s : slots_) {
    if (s->finish_stream) { (void)hipStreamSynchronize((hipStream_t)s->finish_stream); (void)hipStreamDestroy((hipStream_t)s->finish_stream); }
    s->batch.reset();
    for (void* e : {s->uploaded, s->lf_done, s->front_done, s->hf_done, s->idct_done, s->rest_done}) if (e) (void)hipEventDestroy((hipEvent_t)e);
  }
  slots_.clear();
  if (big_.p) DeviceArenaGive(big_.p, big_.cap, device_);
  for (auto& c : coef_) if (c.p) DeviceArenaGive(c.p, c.cap, device_);
  if (clock_event_) (void)hipEventDestroy((hipEvent_t)clock_event_);
  for (void* e : lf_side_done_) if (e) (void)hipEventDestroy((hipEvent_t)e);
  for (void* s : lf_side_) (void)hipStreamDestroy((hipStream_t)s);
  for (void* s : hf_side_) (void)hipStreamDestroy((hipStream_t)s);
  (void)hipStreamDestroy((hipStream_t)upload_);
  (void)hipStreamDestroy((hipStream_t)main_);
  for (void* s : d2h_) (void)hipStreamDestroy((hipStream_t)s);
}

// (device idle as far as these planes go) makes sp a block of at least `bytes`: from the arena pool, else from the runtime
void Pipeline::ReservePlanes(SharedPlanes* sp, size_t bytes) {
  if (sp->p && sp->cap >= bytes) return;
  if (sp->p) { DeviceArenaGive(sp->p, sp->cap, device_, /*idle=*/true); sp->p = nullptr; sp->cap = 0; }
  if (!bytes) return;
  const size_t want = bytes + bytes / 16;
  size_t cap = 0;
  void* p = DeviceArenaTake(want, &cap, device_);
  if (!p) {
    if (hipMalloc(&p, want) != hipSuccess) {
      (void)hipGetLastError();
      DeviceArenaPoolTrim();
      HIP_CHECK(hipMalloc(&p, want));
    }
    cap = want;
  }
  sp->p = (uint8_t*)p; sp->cap = cap; sp->dirty = true; sp->clean_extent = 0;
}

void Pipeline::GrowSharedWhenIdle() {
  // (mu_ held; every job submitted so far has been harvested: nothing on the GPU refers to the shared planes)
  if (want_big_ > big_.cap) ReservePlanes(&big_, want_big_);
  for (auto& c : coef_) if (want_coef_ > c.cap) ReservePlanes(&c, want_coef_);
}

Pipeline::Job* Pipeline::FindJob(int64_t ticket) {
  auto it = jobs_.find(ticket);
  return it == jobs_.end() ? nullptr : it->second.get();
}

int64_t Pipeline::Submit(const uint8_t* const* datas, const size_t* sizes, int n, const OutputSpec& spec, void* const* device_out, void* const* host_out, const size_t* out_capacity,
                         const OutputSpec* each, bool jpeg_pixels) {
  if (n <= 0 || !datas || !sizes) throw ParseError("JxlHipPipelineSubmit: no images", false);
  if (!device_out == !host_out) throw ParseError("JxlHipPipelineSubmit: exactly one of device_out / host_out must be given", false);
  if (jpeg_pixels) {
    bool scaled = spec.downscale != 1;
    for (int i = 0; each && i < n; i++) scaled |= each[i].downscale != 1;
    if (scaled) throw ParseError("JxlHipPipelineSubmitJpegPixels: unsupported: libjpeg-exact decode of an output with downscale 8 (libjpeg's scaled IDCTs are other arithmetic)", true);
  }
  {
    // libjpeg's scaled decodes (OutputSpec::jpeg_scale): one scale per job, and only the libjpeg-exact decode writes such an output
    const uint32_t js = spec.jpeg_scale;
    if (js != 1 && js != 2 && js != 4 && js != 8) throw ParseError("JxlHipPipelineSubmit: jpeg_scale must be 1, 2, 4 or 8", false);
    for (int i = 0; each && i < n; i++)
      if (each[i].jpeg_scale != js) throw ParseError("JxlHipPipelineSubmit: image " + std::to_string(i) + " asks for jpeg_scale " + std::to_string(each[i].jpeg_scale) + ", the job for " + std::to_string(js) + ": one scale per job", false);
    if (js != 1 && !jpeg_pixels) throw ParseError("JxlHipPipelineSubmit: unsupported: jpeg_scale " + std::to_string(js) + " in a job that is not a libjpeg-exact one (only that decode writes libjpeg's scaled picture)", true);
  }
  std::shared_ptr<Job> job(new Job());
  job->datas.assign(datas, datas + n); job->sizes.assign(sizes, sizes + n);
  if (device_out) job->device_out.assign(device_out, device_out + n);
  if (host_out) job->host_out.assign(host_out, host_out + n);
  if (out_capacity) job->capacity.assign(out_capacity, out_capacity + n);
  job->spec = spec; job->spec.device_ptr = nullptr;
  if (each) job->each.assign(each, each + n);
  job->kind = jpeg_pixels ? kJpegPixels : kPlain;
  job->jpeg_region = jpeg_pixels && jpeg_region_.load();      // (the option as it stands at the submit)
  return Enqueue(job, n);
}

int64_t Pipeline::SubmitJpegs(const uint8_t* const* datas, const size_t* sizes, int n, uint32_t flags) {
  if (n <= 0 || !datas || !sizes) throw ParseError("JxlHipPipelineSubmitJpegs: no images", false);
  if (flags & ~(kPipelineJpegDeviceProgressive | kPipelineJpegHostWriter)) throw ParseError("JxlHipPipelineSubmitJpegs: unknown flag bits", false);
  std::shared_ptr<Job> job(new Job());
  job->datas.assign(datas, datas + n); job->sizes.assign(sizes, sizes + n);
  job->kind = kJpegFiles; job->jpeg_flags = flags;
  job->jpeg_files.resize((size_t)n);
  job->result.jpeg_sizes.assign((size_t)n, 0);
  return Enqueue(job, n);
}

int64_t Pipeline::Enqueue(const std::shared_ptr<Job>& job, int n) {
  job->result.status.assign((size_t)n, 1); job->result.error.assign((size_t)n, std::string());
  std::unique_lock<std::mutex> lock(mu_);
  if (shutdown_) throw ParseError("JxlHipPipelineSubmit: the pipeline is shutting down", false);
  // back-pressure: at most nbuf - 1 jobs between submission and the issue of their tail (the issuer's progress never depends on anybody calling Wait)
  cv_.wait(lock, [&] { return shutdown_ || next_ticket_ - next_issue_ < nbuf_ - 1; });
  if (shutdown_) throw ParseError("JxlHipPipelineSubmit: the pipeline is shutting down", false);
  bool idle = next_issue_ == next_ticket_;
  if (idle) for (auto& kv : jobs_) if (kv.second->state != kHarvested) { idle = false; break; }
  if (idle) {
    DeviceScope scope(device_);
    GrowSharedWhenIdle();
    cold_count_ = 0;
  }
  job->ticket = next_ticket_++;
  {
    // the first jobs of a cold pipeline take the one-wavefront-per-stream LF kernel — one after the other: job k's LF stage waits for job k - 1's (on the device), so that the first
    // job's front is done after one kernel time instead of all of them after four (small jobs — latency mode — are wide too, but never chained: they overlap)
    const bool cold = cold_count_ < opt_.wide_first && n > opt_.small_job_frames;
    static const bool no_chain = getenv("JXL_HIP_NO_WIDE_CHAIN") != nullptr;
    job->wide_chain = cold && !no_chain;
    job->wide_after = job->wide_chain && cold_count_ > 0 ? job->ticket - 1 : -1;
    job->cold_wide = cold_count_++ < opt_.wide_first || n <= opt_.small_job_frames;
  }
  // results nobody collects: keep a bounded history
  while (jobs_.size() > (size_t)(8 * nbuf_ + 64)) {
    auto it = jobs_.begin();
    if (it->second->state != kHarvested) break;
    if (it->second->done_event) (void)hipEventDestroy((hipEvent_t)it->second->done_event);
    jobs_.erase(it);
  }
  jobs_[job->ticket] = job;
  prep_queue_.push_back(job);
  lock.unlock();
  cv_.notify_all();
  return job->ticket;
}

void Pipeline::PrepareWorker(int worker) {
  (void)hipSetDevice(device_);
  for (;;) {
    std::shared_ptr<Job> job;
    {
      std::unique_lock<std::mutex> lock(mu_);
      cv_.wait(lock, [&] { return shutdown_ || !prep_queue_.empty(); });
      if (shutdown_) return;
      job = prep_queue_.front(); prep_queue_.pop_front();
      job->state = kPreparing;
    }
    // the slot's previous job must have left the GPU: its batch object is about to be refilled
    if (job->ticket >= nbuf_) {
      std::shared_ptr<Job> prev;
      {
        std::unique_lock<std::mutex> lock(mu_);
        const int64_t pt = job->ticket - nbuf_;
        cv_.wait(lock, [&] { if (shutdown_) return true; auto it = jobs_.find(pt); return it == jobs_.end() || it->second->state >= kTailIssued; });
        if (shutdown_) return;
        auto it = jobs_.find(pt);
        if (it != jobs_.end()) prev = it->second;
      }
      if (prev) Harvest(prev.get());
      else {
        // (collected and dropped already: its Wait harvested it)
      }
    }
    PrepareJob(job.get(), worker);
    { std::lock_guard<std::mutex> lock(mu_); job->state = kPrepared; /* (also when its prepare failed: the LF issuer passes it on) */ }
    cv_.notify_all();
  }
}

void Pipeline::PrepareJob(Job* j, int worker) {
  const auto t0 = std::chrono::steady_clock::now();
  auto t_parse = t0, t_prep = t0;
  Slot& s = *slots_[(size_t)(j->ticket % nbuf_)];
  Batch& bt = *s.batch;
  const int n = (int)j->datas.size();
  try {
    HIP_CHECK(hipSetDevice(device_));
    bt.Reset();
    bt.SetJpegRegion(j->kind == kJpegPixels && j->jpeg_region);      // (before the outputs are set; the slot's batch serves jobs of every kind)
    vec<int> index;
    std::vector<std::string> errors;
    // (a 1:8 job needs the LF part of a stream only; what that decode does not take fails alone, here.  So does a libjpeg-exact job at scale 1/8 for its DC-only images,
    // Batch::JpegDcOnly: a stream that ends behind its LF part and is not one of those fails alone, "truncated")
    bt.AddImagesTolerant(j->datas.data(), j->sizes.data(), n, opt_.parse_threads, &index, &errors, /*for_downscale=*/j->spec.downscale == 8,
                         /*for_jpeg_dc=*/j->kind == kJpegPixels && j->spec.jpeg_scale == 8);
    t_parse = std::chrono::steady_clock::now();
    j->batch_index.assign(index.begin(), index.end());
    bool any = false;
    const bool files = j->kind == kJpegFiles;
    if (files) {
      // a reconstruction job: no outputs.  What the batch call refuses fails alone here, with that call's text, and stays in the batch (its frame is never consumed:
      // EnqueueJpegPlan below sets its status word, so that the HF stage puts zeros back behind it); a job without one image to reconstruct never reaches the GPU
      bt.jpeg_host_writer = (j->jpeg_flags & kPipelineJpegHostWriter) != 0;
      bt.jpeg_device_progressive = (j->jpeg_flags & kPipelineJpegDeviceProgressive) != 0;
      for (int i = 0; i < n; i++) {
        const int bi = index[(size_t)i];
        if (bi < 0) { j->result.error[(size_t)i] = errors[(size_t)i]; continue; }
        std::string why;
        if (bt.CanReconstructJpeg(bi, &why)) any = true;
        else { j->result.error[(size_t)i] = "JPEG reconstruction: " + why; j->batch_index[(size_t)i] = -2 - bi; }
      }
      if (!any) { j->job_error = "JPEG reconstruction: no image of the job can be reconstructed"; return; }
    }
    for (int i = 0; i < n && !files; i++) {
      if (index[(size_t)i] < 0) { j->result.error[(size_t)i] = errors[(size_t)i]; continue; }
      OutputSpec o = j->each.empty() ? j->spec : j->each[(size_t)i];
      o.device_ptr = j->device_out.empty() ? nullptr : j->device_out[(size_t)i];
      // (an image the libjpeg-exact decode does not take has no scaled picture: it stays in the batch at scale 1, unwritten, and fails with that decode's reason below)
      if (j->kind == kJpegPixels && o.jpeg_scale != 1 && !bt.CanDecodeJpegPixels(index[(size_t)i], nullptr)) o.jpeg_scale = 1;
      // (nor a u8 picture for the integer resample, OutputSpec::resize_u8: it stays as an f32-resampled output, unwritten, and fails alone with the reason below)
      const bool wants_u8 = o.resize_u8;
      if (j->kind == kJpegPixels && o.resize_u8 && !bt.CanDecodeJpegPixels(index[(size_t)i], nullptr)) o.resize_u8 = false;
      size_t need = 0;
      std::string refusal;
      try { need = bt.OutputSizeOf(index[(size_t)i], o); } catch (const ParseError& e) { refusal = e.what(); }     // (a plane_stride this image does not fit, a crop that leaves it: Batch::LayoutRefusal / ResizeRefusal)
      std::string not_eligible;
      if (!refusal.empty()) {
        // (stays in the batch like an image whose buffer is too small, with a tight plane of its own and no crop, mirror or filter)
        j->result.error[(size_t)i] = refusal;
        o.device_ptr = nullptr; o.plane_stride = 0; o.crop_x0 = o.crop_y0 = o.crop_w = o.crop_h = 0; o.mirror = false; o.resize_filter = 0; o.planes = OutputPlanes(); o.color_set = false;
        j->batch_index[(size_t)i] = -2 - index[(size_t)i];
      } else if (j->kind == kJpegPixels && !bt.CanDecodeJpegPixels(index[(size_t)i], &not_eligible)) {
        // (a libjpeg-exact job: what that decode does not take stays in the batch too and fails with the batch call's reason; nothing is written for it)
        j->result.error[(size_t)i] = wants_u8 ? "unsupported: integer resample of an image the libjpeg-exact decode does not take (" + not_eligible + ")" : not_eligible;
        o.device_ptr = nullptr;
        j->batch_index[(size_t)i] = -2 - index[(size_t)i];
      } else if (!j->capacity.empty() && j->capacity[(size_t)i] < need) {
        // (the image stays in the batch — taking it out would renumber the others — and decodes into a buffer of the batch's own; it is reported as failed)
        j->result.error[(size_t)i] = "output buffer too small for this image";
        o.device_ptr = nullptr;
        j->batch_index[(size_t)i] = -2 - index[(size_t)i];
      } else if ((!j->device_out.empty() && !j->device_out[(size_t)i]) || (!j->host_out.empty() && !j->host_out[(size_t)i])) {
        j->result.error[(size_t)i] = "no output buffer for this image";
        o.device_ptr = nullptr;
        j->batch_index[(size_t)i] = -2 - index[(size_t)i];
      } else any = true;
      bt.SetOutput(index[(size_t)i], o);
    }
    if (!any) { j->job_error = "no image of the job could be parsed"; return; }
    bt.cfg.lane_stride_lf = opt_.lane_stride_lf; bt.cfg.lane_stride_hf = opt_.lane_stride_hf; bt.cfg.no_flag_wait = opt_.no_flag_wait;
    // latency mode: sparse wavefronts in the SIMT HF stage — one group stream per wavefront for a handful of frames, four up to a hundred (kernels.hip LaunchHfDecode)
    bt.cfg.hf_lanes_per_wave = bt.cfg.hf_lanes_per_wg = 0;
    if (opt_.hf_sparse || n <= opt_.small_job_frames) {
      if (n <= 8) { bt.cfg.hf_lanes_per_wave = 1; bt.cfg.hf_lanes_per_wg = 16; }
      else if (n <= 96) { bt.cfg.hf_lanes_per_wave = 4; bt.cfg.hf_lanes_per_wg = 64; }
    }
    bt.UseSharedPlanes(&big_, &coef_[(size_t)(j->ticket % ncoef_)]);
    // tables + upload start at once, on the upload stream: the job's LF stage — enqueued by the LF issuer, perhaps with other jobs' — waits for `uploaded` on the device
    void* side = upload_;
    bt.Prepare(side, /*wait_upload=*/false);
    size_t jpeg_table = 0;
    if (files) {
      // the host plan of the reconstruction; scan table, tables, resets and gather table travel on the stream of the LF stage.  What Prepare alone could tell (the
      // quantisation table of a one-group frame) fails its image here.
      const size_t left = bt.PlanJpegWrite();
      for (int i = 0; i < n; i++) {
        const int bi = index[(size_t)i];
        if (bi < 0 || j->batch_index[(size_t)i] < 0) continue;
        const Batch::JpegResult* r = bt.jpeg_result(bi);
        if (r && !r->error.empty()) { j->result.error[(size_t)i] = r->error; j->batch_index[(size_t)i] = -2 - bi; }
      }
      if (!left) throw ParseError("JPEG reconstruction: no image of the job can be reconstructed", true);
      bt.EnqueueJpegPlan(side, /*fail_refused=*/true);
    }
    if (j->kind == kJpegPixels) {
      // the host plan of the libjpeg-exact tail; its table travels on the stream of the LF stage.  What Prepare alone could tell (the quantisation table of a
      // one-group frame, a block grid that does not hold the image) fails its image here.
      jpeg_table = bt.PlanJpegPixels();
      for (int i = 0; i < n; i++) {
        const int bi = index[(size_t)i];
        if (bi < 0 || j->batch_index[(size_t)i] < 0) continue;
        const Batch::JpegPixelResult* r = bt.jpeg_pixel_result(bi);
        if (r && !r->error.empty()) { j->result.error[(size_t)i] = r->error; j->batch_index[(size_t)i] = -2 - bi; }
      }
      bt.EnqueueJpegPixelTable(side, /*fail_refused=*/true);
    }
    t_prep = std::chrono::steady_clock::now();
    {
      std::lock_guard<std::mutex> lock(mu_);
      last_info_["jpeg_pixel_images"] = (int64_t)jpeg_table;
      last_info_["jpeg_pixel_launches"] = j->kind == kJpegPixels ? (int64_t)bt.jpeg_pixel_launch_count() : 0;
      last_info_["hf_groups_total"] = j->kind == kJpegPixels ? bt.Info("hf_groups_total") : 0; last_info_["hf_groups_decoded"] = j->kind == kJpegPixels ? bt.Info("hf_groups_decoded") : 0;
      want_big_ = std::max(want_big_, bt.big_bytes_wanted()); want_coef_ = std::max(want_coef_, bt.coef_bytes_wanted());
      if (!bt.uses_shared_big() || !bt.uses_shared_coef()) private_plane_jobs_++;
      bt.StageBytes(last_stage_bytes_);
      for (const char* k : {"lf_simt_frames", "lf_legacy_frames", "lf_simt_wp", "lf_simt_lanes", "lf_simt_waves"}) last_info_[k] = bt.Info(k);
      last_info_["compressed_bytes"] = (int64_t)bt.compressed_bytes();
      last_info_["total_pixels"] = (int64_t)bt.total_pixels();
      last_info_["frames"] = (int64_t)bt.size();
    }
    // the first LF stages of a cold pipeline, and small jobs, take the one-wavefront-per-stream kernel (read by the LF issuer: such a job never shares a launch)
    if (j->cold_wide && opt_.lane_stride_lf < 64) bt.cfg.lf_wide_once = 1;
    Record(s.uploaded, side);
  } catch (const std::exception& e) {
    j->job_error = e.what();
    if (j->job_error.empty()) j->job_error = "prepare failed";
  }
  const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  static const bool trace = getenv("JXL_HIP_SCHED_TRACE") != nullptr;
  if (trace) fprintf(stderr, "[pipe %.1f] job %lld (%d images, slot %d): prepare %.1f ms (parse %.1f, prepare %.1f)%s%s\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(),
                     (long long)j->ticket, n, (int)(j->ticket % nbuf_), dt * 1e3, std::chrono::duration<double, std::milli>(t_parse - t0).count(), std::chrono::duration<double, std::milli>(t_prep - t_parse).count(), j->job_error.empty() ? "" : " ERROR ", j->job_error.c_str());
  std::lock_guard<std::mutex> lock(mu_);
  prepare_s_total_ += dt; prepared_jobs_++;
}

// The LF stages of every job, from one thread, in ticket order.  The thread takes the next LF stream round robin, waits (host) until the group before on that stream has
// left the GPU, and then takes along every job that is ready by then and that PlanLfGroups puts into the first group: while streams are free every job leaves alone, the
// moment it is prepared; when LF launches are the bottleneck the jobs that queued up meanwhile share one launch, which takes about as long as a launch for one of them.
void Pipeline::LfIssuerLoop() {
  (void)hipSetDevice(device_);
  size_t turn = 0;
  auto ready = [&](int64_t t) { auto it = jobs_.find(t); return it != jobs_.end() && it->second->state == kPrepared; };
  for (;;) {
    void* stream = nullptr; void* busy = nullptr;
    {
      std::unique_lock<std::mutex> lock(mu_);
      cv_.wait(lock, [&] { return shutdown_ || ready(next_lf_); });
      if (shutdown_) return;
      const size_t in_use = (size_t)LfStreamsInUse();
      try {
        while (lf_side_.size() < in_use) { lf_side_.push_back(NewStream(prio_high_)); lf_side_done_.push_back(nullptr); }      // (an option raised the number)
      } catch (const std::exception&) {}
      turn %= std::min(in_use, lf_side_.size());
      stream = lf_side_[turn]; busy = lf_side_done_[turn];
    }
    if (busy) (void)hipEventSynchronize((hipEvent_t)busy);
    std::vector<std::shared_ptr<Job>> group;
    {
      std::lock_guard<std::mutex> lock(mu_);
      if (shutdown_) return;
      std::vector<std::shared_ptr<Job>> cand;
      std::vector<LfGroupKey> keys;
      for (int64_t t = next_lf_; (int)cand.size() < kLfGroupMax && ready(t); t++) {
        cand.push_back(jobs_[t]);
        Job& j = *cand.back();
        // (a job whose prepare failed has nothing to launch; reconstruction and libjpeg-exact jobs keep a launch of their own)
        keys.push_back(j.job_error.empty() && j.kind == kPlain ? slots_[(size_t)(j.ticket % nbuf_)]->batch->LfKey() : LfGroupKey());
      }
      const int m = PlanLfGroups(keys.data(), (int)keys.size(), lf_group_max_.load())[0];
      group.assign(cand.begin(), cand.begin() + m);
    }
    IssueLfGroup(group, stream);
    {
      std::lock_guard<std::mutex> lock(mu_);
      try {
        if (!lf_side_done_[turn]) lf_side_done_[turn] = NewEvent();
        Record(lf_side_done_[turn], stream);
      } catch (const std::exception&) {}
      int launched = 0;
      for (auto& j : group) { j->state = kFrontIssued; launched += j->job_error.empty(); }
      if (launched) { lf_groups_++; lf_grouped_jobs_ += launched; lf_group_largest_ = std::max<int64_t>(lf_group_largest_, launched); }
      next_lf_ += (int64_t)group.size();
    }
    cv_.notify_all();
    turn++;
  }
}

void Pipeline::IssueLfGroup(const std::vector<std::shared_ptr<Job>>& group, void* stream) {
  std::vector<Job*> live;
  std::vector<Batch*> batches;
  size_t done = 0;        // members whose front is in the stream
  try {
    for (auto& jp : group) {
      Job* j = jp.get();
      if (!j->job_error.empty()) continue;
      Slot& s = *slots_[(size_t)(j->ticket % nbuf_)];
      Batch& bt = *s.batch;
      StreamWait(stream, s.uploaded);
      // (jobs whose LF trees use the weighted predictor keep the SIMT kernel whatever lf_wide_once says — LaunchLfDecode —: 420 ms a launch, nothing to chain)
      static const bool wide_wp = getenv("JXL_HIP_WIDE_WP") != nullptr;       // experiments (kernels.hip LfSimtShapeOf)
      const bool lf_wide = bt.cfg.lf_wide_once && (wide_wp || !bt.Info("lf_simt_wp"));
      bool chained = false;
      {
        std::lock_guard<std::mutex> lock(mu_);
        if (j->wide_chain) j->lf_wide = lf_wide;
        if (j->wide_after >= 0 && lf_wide) {
          // behind the cold-start job before it, whose LF stage this thread has enqueued already: ours waits for it on the device
          auto it = jobs_.find(j->wide_after);
          chained = it != jobs_.end() && it->second->job_error.empty() && it->second->state < kHarvested && it->second->lf_wide;
        }
      }
      if (chained) StreamWait(stream, slots_[(size_t)(j->wide_after % nbuf_)]->lf_done);
      live.push_back(j); batches.push_back(&bt);
    }
    if (live.empty()) return;
    const bool timed = opt_.timed != 0 && live[0]->kind != kJpegFiles;   // (a reconstruction job has no pixel stages to bracket: its parts are not timed; it is a group of its own)
    Batch::RunLfGroup(batches.data(), (int)batches.size(), stream, timed, [&](int i) {
      // LF decode + varblock placement are in the stream: all the HF stage waits for
      Job* j = live[(size_t)i];
      Slot& s = *slots_[(size_t)(j->ticket % nbuf_)];
      Record(s.lf_done, stream);
      // LF post-processing: needed by the float IDCT and the filters only — the libjpeg-exact tail and the reconstruction's gather read lfq, the coefficient planes, block info and offsets, the
      // chroma-from-luma maps: nothing LfDequantKernel, LfSmoothKernel, LlfSigmaKernel or LlfKernel write (lf, lf_tmp, llf, inv_sigma)
      s.batch->RunPart(stream, PartOf(kStageLfPost, j->kind != kPlain), timed);
      Record(s.front_done, stream);
      done = (size_t)i + 1;
    });
  } catch (const std::exception& e) {
    // what is in the stream keeps those slots busy (Harvest drains the streams of a failed job); the members behind the failure fail with it
    const std::string why = *e.what() ? e.what() : "LF stage failed";
    std::lock_guard<std::mutex> lock(mu_);
    for (auto& jp : group)
      if (jp->job_error.empty() && std::find(live.begin(), live.begin() + (ptrdiff_t)done, jp.get()) == live.begin() + (ptrdiff_t)done) jp->job_error = why;
  }
}

void Pipeline::IssueHf(Job* j) {
  if (j->hf_issued) return;
  j->hf_issued = true;
  if (!j->job_error.empty()) return;
  Slot& s = *slots_[(size_t)(j->ticket % nbuf_)];
  void* hs = hf_side_[(size_t)(j->ticket % (int64_t)hf_side_.size())];
  try {
    StreamWait(hs, s.lf_done);
    // the coefficient set's previous user has consumed (and zeroed) it: its tail was issued before this call (tails go out in order, HF stages at most hf_streams ahead)
    if (j->ticket >= ncoef_) StreamWait(hs, slots_[(size_t)((j->ticket - ncoef_) % nbuf_)]->idct_done);
    // (a libjpeg-exact job: part 12, the HF stage that honours the group lists of images decoded by region)
    s.batch->RunPart(hs, PartOf(kStageHf, j->kind == kJpegPixels), opt_.timed != 0 && j->kind != kJpegFiles);
    Record(s.hf_done, hs);
  } catch (const std::exception& e) { j->job_error = e.what(); }
}

void Pipeline::IssueTail(Job* j) {
  Slot& s = *slots_[(size_t)(j->ticket % nbuf_)];
  Batch& bt = *s.batch;
  if (j->job_error.empty()) {
    try {
      StreamWait(main_, s.hf_done);
      StreamWait(main_, s.front_done);
      // IDCT (float, or the integer one over the HF planes; a reconstruction job: the gather into the JPEG writer's arena): the last stage that touches the coefficient
      // set, which is clean behind it
      if (j->kind == kJpegFiles) bt.EnqueueJpegGather(main_); else bt.RunPart(main_, PartOf(kStageIdct, j->kind == kJpegPixels), opt_.timed != 0);
      Record(s.idct_done, main_);
      // restoration filters, colour, write (libjpeg-exact jobs: chroma upsampling, colour, write); resizes.  A reconstruction job: the sizes pass of the writer — its
      // pack pass, sized on the host from what that pass found, and the splice belong to the harvest
      if (j->kind == kJpegFiles) bt.EnqueueJpegSizes(main_); else bt.RunPart(main_, PartOf(kStagePixels, j->kind == kJpegPixels), opt_.timed != 0);
      Record(s.rest_done, main_);
      void* d2h = d2h_[0];
      StreamWait(d2h, s.rest_done);
      if (j->kind == kJpegFiles) bt.EnqueueJpegHeadReadback(d2h);      // the raw size and the flag words travel with the status words
      if (!j->host_out.empty()) {
        // equally sized images at equal distances on both sides (a job of same-shaped frames into one host buffer): one pitched copy instead of one per image
        bool pitched = j->host_out.size() >= 2;
        ptrdiff_t hp = 0, dp = 0;
        size_t osz = 0;
        for (size_t i = 0; i < j->host_out.size() && pitched; i++) {
          const int bi = j->batch_index[i];
          if (bi < 0) { pitched = false; break; }
          if (i == 0) { osz = bt.image(bi).out_size; continue; }
          const ptrdiff_t h = (const uint8_t*)j->host_out[i] - (const uint8_t*)j->host_out[i - 1];
          const ptrdiff_t d = (const uint8_t*)bt.device_output(bi) - (const uint8_t*)bt.device_output(j->batch_index[i - 1]);
          if (i == 1) { hp = h; dp = d; }
          if (h != hp || d != dp || bt.image(bi).out_size != osz || hp < (ptrdiff_t)osz || dp < (ptrdiff_t)osz) pitched = false;
        }
        static const bool no_pitched = getenv("JXL_HIP_NO_PITCHED_D2H") != nullptr;
        if (pitched && !no_pitched) {
          HIP_CHECK(hipMemcpy2DAsync(j->host_out[0], (size_t)hp, bt.device_output(j->batch_index[0]), (size_t)dp, osz, j->host_out.size(), hipMemcpyDeviceToHost, (hipStream_t)d2h));
        } else {
          for (size_t i = 0; i < j->host_out.size(); i++) {
            const int bi = j->batch_index[i];
            if (bi < 0) continue;
            HIP_CHECK(hipMemcpyAsync(j->host_out[i], bt.device_output(bi), bt.image(bi).out_size, hipMemcpyDeviceToHost, (hipStream_t)d2h));
          }
        }
      }
      bt.EnqueueStatusReadback(d2h);
    } catch (const std::exception& e) {
      j->job_error = e.what();
      // whatever was enqueued keeps the slot busy: Harvest drains the streams before the batch object is touched again
    }
  } else {
    // (nothing was enqueued beyond the front — if that; the events of this slot keep the state of its previous job, which completed long ago)
    try { Record(s.idct_done, main_); Record(s.rest_done, main_); } catch (...) {}
  }
  try {
    if (!j->done_event) j->done_event = NewEvent(true);
    Record(j->done_event, d2h_[0]);
  } catch (const std::exception& e) { if (j->job_error.empty()) j->job_error = e.what(); }
}

void Pipeline::IssuerLoop() {
  (void)hipSetDevice(device_);
  for (;;) {
    std::shared_ptr<Job> job;
    std::vector<std::shared_ptr<Job>> ahead;
    {
      std::unique_lock<std::mutex> lock(mu_);
      cv_.wait(lock, [&] { if (shutdown_) return true; auto it = jobs_.find(next_issue_); return it != jobs_.end() && it->second->state >= kFrontIssued; });
      if (shutdown_) return;
      job = jobs_[next_issue_];
      for (int a = 1; a <= opt_.hf_streams; a++) {
        auto it = jobs_.find(next_issue_ + a);
        if (it == jobs_.end() || it->second->state < kFrontIssued) break;       // (its LF stage is not enqueued yet: the events it would wait for are a previous job's)
        ahead.push_back(it->second);
      }
    }
    IssueHf(job.get());
    for (auto& a : ahead) IssueHf(a.get());
    IssueTail(job.get());
    { std::lock_guard<std::mutex> lock(mu_); job->state = kTailIssued; next_issue_++; }
    cv_.notify_all();
  }
}

void Pipeline::Harvest(Job* j) {
  Slot& s = *slots_[(size_t)(j->ticket % nbuf_)];
  std::lock_guard<std::mutex> slot_lock(s.mu);
  { std::lock_guard<std::mutex> lock(mu_); if (j->state >= kHarvested) return; }
  DeviceScope scope(device_);
  Batch& bt = *s.batch;
  const size_t n = j->datas.size();
  bool readback_ok = false;
  vec<uint32_t> st;
  if (j->job_error.empty()) {
    try { bt.HarvestStatus(&st); if (j->kind == kJpegPixels) bt.HarvestJpegPixels(st); readback_ok = true; } catch (const std::exception& e) { j->job_error = e.what(); }
  }
  bool finish_failed = false;
  double finish_ms = 0;
  if (j->kind == kJpegFiles && readback_ok) {
    const auto f0 = std::chrono::steady_clock::now();
    // pack pass, copies and splice of THIS job, on a stream no other job's stages queue behind, in the thread that collects it (or the prepare thread that takes over
    // its slot) — while the issuer goes on with the entropy stages of the jobs behind it
    try {
      if (!s.finish_stream) s.finish_stream = NewStream(0);
      bt.FinishJpegWrite(s.finish_stream, st);
      if (j->done_event) Record(j->done_event, s.finish_stream);        // end_ms: behind the last copy of the finish phase
      static const char* const kCounts[4] = {"jpeg_device_images", "jpeg_host_images", "jpeg_device_progressive_images", "jpeg_gather_launches"};
      for (int k = 0; k < 4; k++) j->jpeg_counts[k] = bt.Info(kCounts[k]);
    } catch (const std::exception& e) { j->job_error = e.what(); finish_failed = true; }
    finish_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - f0).count();
  }
  if (j->done_event) {
    (void)hipEventSynchronize((hipEvent_t)j->done_event);
    float ms = 0;
    if (hipEventElapsedTime(&ms, (hipEvent_t)clock_event_, (hipEvent_t)j->done_event) == hipSuccess) j->result.end_ms = ms; else (void)hipGetLastError();
  }
  if (finish_failed && s.finish_stream) (void)hipStreamSynchronize((hipStream_t)s.finish_stream);
  if (!j->job_error.empty() && !readback_ok) {
    // a job that failed half-way: whatever it enqueued must have left the GPU before the slot is reused
    (void)hipStreamSynchronize((hipStream_t)main_);
    (void)hipStreamSynchronize((hipStream_t)upload_);
    std::vector<void*> lf_now;
    { std::lock_guard<std::mutex> lock(mu_); lf_now = lf_side_; }      // (the LF issuer adds streams under mu_ when an option raises their number)
    for (void* x : lf_now) (void)hipStreamSynchronize((hipStream_t)x);
    for (void* x : hf_side_) (void)hipStreamSynchronize((hipStream_t)x);
    for (void* x : d2h_) (void)hipStreamSynchronize((hipStream_t)x);
  }
  for (size_t i = 0; i < n; i++) {
    const int bi = i < j->batch_index.size() ? j->batch_index[i] : -1;
    if (!j->result.error[i].empty()) { j->result.status[i] = 1; continue; }
    if (!j->job_error.empty() || bi < 0) { j->result.status[i] = 1; j->result.error[i] = j->job_error.empty() ? "not decoded" : j->job_error; continue; }
    if (j->kind == kJpegFiles) {
      // (a damaged stream: FinishJpegWrite has named the status word, as the batch call does)
      Batch::JpegResult* r = bt.mutable_jpeg_result(bi);
      if (r && r->ok) { j->result.status[i] = 0; j->result.jpeg_sizes[i] = r->bytes.size(); j->jpeg_files[i] = std::move(r->bytes); r->bytes.clear(); }
      else { j->result.status[i] = 1; j->result.error[i] = r && !r->error.empty() ? r->error : "JPEG reconstruction: no file"; }
      continue;
    }
    uint32_t bad = 0;
    for (int u = bt.first_unit_of(bi); u < bt.first_unit_of(bi) + bt.num_units_of(bi); u++) bad |= st[(size_t)u];
    if (bad) {
      j->result.status[i] = 1;
      const Batch::JpegPixelResult* jr = j->kind == kJpegPixels ? bt.jpeg_pixel_result(bi) : nullptr;
      if (jr && !jr->error.empty()) j->result.error[i] = jr->error;      // (names what JpegIdctPlanesKernel refused: a transform other than DCT8)
      else j->result.error[i] = (bad & kErrUnsupported) ? "unsupported: stream feature on the device path" : "corrupt stream (device status " + std::to_string(bad) + ")";
    } else j->result.status[i] = 0;
  }
  static const bool trace = getenv("JXL_HIP_SCHED_TRACE") != nullptr;
  if (trace && readback_ok && j->kind == kJpegFiles)
    fprintf(stderr, "[pipe %.1f] job %lld (reconstruction, %zu images): status words in hand, then pack pass + copies + splice %.1f ms on the collecting thread; done at %.1f ms\n",
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(), (long long)j->ticket, n, finish_ms, j->result.end_ms);
  if (trace && opt_.timed && readback_ok && j->kind != kJpegFiles) {
    float tl[kNumMarks];
    bt.DebugTimeline(clock_event_, tl);
    fprintf(stderr, "[pipe] job %lld timeline (ms): LF %.1f .. %.1f, LF post end %.1f, HF %.1f .. %.1f, IDCT %.1f .. %.1f, filters end %.1f, out end %.1f\n", (long long)j->ticket, tl[kMarkLfStart], tl[kMarkLfEnd], tl[kMarkLfPostEnd], tl[kMarkHfStart], tl[kMarkHfEnd],
            tl[kMarkIdctStart], tl[kMarkIdctEnd], tl[kMarkFiltersEnd], tl[kMarkOutputEnd]);
    int runs = 0;
    const StageTimes t = bt.CollectTimes(&runs);
    fprintf(stderr, "[pipe] job %lld (%zu images) on the GPU: lf %.1f lfpost %.1f hf %.1f idct %.1f filters %.1f out %.1f, first kernel to last %.1f ms; done at %.1f ms\n", (long long)j->ticket, n, t.lf_ms, t.lfpost_ms,
            t.hf_ms, t.idct_ms, t.filter_ms, t.out_ms, t.total_ms, j->result.end_ms);
  }
  {
    std::lock_guard<std::mutex> lock(mu_);
    if (readback_ok) last_info_["hf_nonzeros"] = bt.Info("hf_nonzeros");
    if (readback_ok) last_info_["resize_u8_images"] = bt.Info("resize_u8_images");     // (of the job harvested last: its images resampled in Pillow's 8-bit arithmetic)
    if (readback_ok) { last_info_["jpeg_pixel_images"] = j->kind == kJpegPixels ? bt.Info("jpeg_pixel_images") : 0; last_info_["jpeg_pixel_launches"] = j->kind == kJpegPixels ? bt.Info("jpeg_pixel_launches") : 0;
                       last_info_["jpeg_dc_only_images"] = j->kind == kJpegPixels ? bt.Info("jpeg_dc_only_images") : 0; }
    if (readback_ok) {
      last_info_["jpeg_device_images"] = j->jpeg_counts[0]; last_info_["jpeg_host_images"] = j->jpeg_counts[1];
      last_info_["jpeg_device_progressive_images"] = j->jpeg_counts[2]; last_info_["jpeg_gather_launches"] = j->jpeg_counts[3];
    }
    j->state = kHarvested;
  }
  cv_.notify_all();
}

std::shared_ptr<Pipeline::Job> Pipeline::WaitIssued(int64_t ticket, const char* who, bool jpegs) {
  std::unique_lock<std::mutex> lock(mu_);
  auto it = jobs_.find(ticket);
  if (it == jobs_.end()) throw ParseError(std::string(who) + ": unknown ticket (never submitted, collected already, or too old)", false);
  std::shared_ptr<Job> job = it->second;
  if (jpegs && job->kind != kJpegFiles) throw ParseError(std::string(who) + ": this ticket is not a reconstruction job's (JxlHipPipelineSubmitJpegs)", false);
  if (job->waited) throw ParseError(std::string(who) + ": this ticket is being waited for already", false);
  job->waited = true;
  cv_.wait(lock, [&] { return shutdown_ || job->state >= kTailIssued; });
  if (job->state < kTailIssued) throw ParseError(std::string(who) + ": the pipeline is shutting down", false);
  return job;
}

void Pipeline::Wait(int64_t ticket, PipelineJobResult* out) {
  std::shared_ptr<Job> job = WaitIssued(ticket, "JxlHipPipelineWait", false);
  Harvest(job.get());
  if (out) *out = job->result;
  std::lock_guard<std::mutex> lock(mu_);
  if (job->done_event) { (void)hipEventDestroy((hipEvent_t)job->done_event); job->done_event = nullptr; }
  jobs_.erase(ticket);          // (a reconstruction job: its files go with it)
}

void Pipeline::WaitJpegs(int64_t ticket, PipelineJobResult* out) {
  std::shared_ptr<Job> job = WaitIssued(ticket, "JxlHipPipelineWaitJpegs", true);
  Harvest(job.get());
  if (out) *out = job->result;
  std::lock_guard<std::mutex> lock(mu_);
  if (job->done_event) { (void)hipEventDestroy((hipEvent_t)job->done_event); job->done_event = nullptr; }
  job->collected = true;        // (stays in jobs_ with its files until ReleaseJpegs)
}

std::shared_ptr<Pipeline::Job> Pipeline::CollectedJpegs(int64_t ticket, int i, const char* who) {
  std::lock_guard<std::mutex> lock(mu_);
  auto it = jobs_.find(ticket);
  if (it == jobs_.end() || it->second->kind != kJpegFiles || !it->second->collected)
    throw ParseError(std::string(who) + ": unknown ticket (not a reconstruction job's, not waited for with JxlHipPipelineWaitJpegs, or released already)", false);
  if (i < 0 || (size_t)i >= it->second->jpeg_files.size()) throw ParseError(std::string(who) + ": no such image", false);
  return it->second;
}
int Pipeline::JpegStatus(int64_t ticket, int i, std::string* error) {
  std::shared_ptr<Job> job = CollectedJpegs(ticket, i, "JxlHipPipelineJpegStatus");
  if (job->result.status[(size_t)i] == 0) return 0;
  if (error) *error = job->result.error[(size_t)i];
  return 1;
}
void Pipeline::CopyJpeg(int64_t ticket, int i, void* dst, size_t capacity) {
  std::shared_ptr<Job> job = CollectedJpegs(ticket, i, "JxlHipPipelineCopyJpeg");
  if (job->result.status[(size_t)i] != 0) throw ParseError(job->result.error[(size_t)i], false);
  const vec<uint8_t>& f = job->jpeg_files[(size_t)i];
  if (!dst || capacity < f.size()) throw ParseError("JxlHipPipelineCopyJpeg: the buffer is smaller than the file", false);
  if (!f.empty()) memcpy(dst, f.data(), f.size());
}
void Pipeline::ReleaseJpegs(int64_t ticket) {
  std::lock_guard<std::mutex> lock(mu_);
  auto it = jobs_.find(ticket);
  if (it == jobs_.end() || it->second->kind != kJpegFiles || !it->second->collected) return;
  jobs_.erase(it);
}

void Pipeline::WaitAll() {
  for (;;) {
    std::shared_ptr<Job> job;
    {
      std::unique_lock<std::mutex> lock(mu_);
      const int64_t upto = next_ticket_;
      cv_.wait(lock, [&] { return shutdown_ || next_issue_ >= upto; });
      for (auto& kv : jobs_) if (kv.second->state == kTailIssued) { job = kv.second; break; }
      if (!job) return;
    }
    Harvest(job.get());
  }
}

void Pipeline::ResetClock() {
  WaitAll();
  std::lock_guard<std::mutex> lock(mu_);
  DeviceScope scope(device_);
  (void)hipStreamSynchronize((hipStream_t)main_);
  Record(clock_event_, main_);
  (void)hipStreamSynchronize((hipStream_t)main_);
  prepare_s_total_ = 0; prepared_jobs_ = 0;
  lf_groups_ = lf_grouped_jobs_ = lf_group_largest_ = 0;
}

StageTimes Pipeline::CollectTimes(int* runs) {
  WaitAll();
  DeviceScope scope(device_);
  StageTimes t; int total = 0;
  for (auto& s : slots_) {
    int r = 0;
    const StageTimes x = s->batch->CollectTimes(&r);
    total += r;
    t.lf_ms += x.lf_ms; t.lfpost_ms += x.lfpost_ms; t.hf_ms += x.hf_ms; t.idct_ms += x.idct_ms; t.filter_ms += x.filter_ms; t.out_ms += x.out_ms; t.total_ms += x.total_ms;
  }
  if (runs) *runs = total;
  return t;
}

void Pipeline::StageBytes(uint64_t out[6]) { std::lock_guard<std::mutex> lock(mu_); for (int i = 0; i < 6; i++) out[i] = last_stage_bytes_[i]; }

int64_t Pipeline::Info(const char* name) {
  const std::string n(name ? name : "");
  std::lock_guard<std::mutex> lock(mu_);
  if (n == "jobs") return next_ticket_;
  if (n == "slots") return nbuf_;
  if (n == "coefficient_sets") return ncoef_;
  if (n == "shared_big_bytes") return (int64_t)big_.cap;
  if (n == "shared_coef_bytes") { int64_t v = 0; for (auto& c : coef_) v += (int64_t)c.cap; return v; }
  if (n == "private_plane_jobs") return private_plane_jobs_;
  if (n == "lf_groups") return lf_groups_;
  if (n == "lf_grouped_jobs") return lf_grouped_jobs_;
  if (n == "lf_group_largest") return lf_group_largest_;
  if (n == "lf_streams_effective") return LfStreamsInUse();
  if (n == "lf_group_max") return lf_group_max_.load();
  if (n == "device_bytes") {
    int64_t v = (int64_t)big_.cap;
    for (auto& c : coef_) v += (int64_t)c.cap;
    for (auto& s : slots_) v += (int64_t)(s->batch->const_bytes() + s->batch->work_bytes());
    return v;
  }
  auto it = last_info_.find(n);
  return it == last_info_.end() ? -1 : it->second;
}

}  // namespace jxlhip

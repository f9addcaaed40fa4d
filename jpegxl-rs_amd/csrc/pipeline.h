// jxl-hip: the streaming decode pipeline of one GPU as a library object (C ABI: JxlHipPipeline*, include/jxl_hip.h).
//
// A decode is LF (entropy decode of the LF groups: a serial chain per stream, hundreds of milliseconds per launch whatever the batch size) ->
// varblock placement + LF post-processing -> HF (entropy decode of the coefficients) -> IDCT -> filters + write.  Throughput comes from jobs in
// flight: while the tail (IDCT, filters, write) of job k runs on the main stream, the HF stage of job k + 1 runs on a stream of its own against
// the other coefficient set, the LF stages of the jobs behind it on side streams, and host worker threads parse, build tables for and upload
// the jobs after those.  One thread enqueues the LF stages, in submission order, on as many LF streams as the hardware queues of the process
// leave room for (streams that share a queue serialise); jobs that became ready while the next LF stream was busy go out as ONE launch of the
// SIMT LF kernel, which is latency-bound and takes about as long for several jobs as for one.  The object owns what that takes: the ring of
// batch objects (their LF-stage outputs), the coefficient sets and the pixel planes all jobs share, the HIP streams and events, the prepare
// threads, the LF issuer and the thread that issues HF stages and tails in submission order.  (Rounds 1-4 kept this schedule in bench.py; it
// is a property of the library now.)
//
// The reference decodes batches by looping decode_with over files (jpegxl-rs/benches/decode.rs:16-19): there is no counterpart of this object
// in the reference API.  The libjxl-compatible JxlDecoder reaches it through DeviceScheduler (scheduler.cc): concurrent decode_with callers of
// one process are coalesced into jobs of one shared pipeline per device.
#pragma once
#include "decoder.h"
#include <atomic>
#include <condition_variable>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

namespace jxlhip {

struct PipelineOptions {
  int in_flight = 11;        // jobs in flight on the GPU (LF stages run this many jobs ahead of the tail, minus one)
  int lf_streams = 11;       // side streams the LF stages are spread over, at most (one per job in flight: weighted-predictor LF stages take ~590 ms per launch against steps of ~75 ms, seven streams bound such frames
                             // at 84 ms per step).  Streams that share a hardware queue serialise, so only as many are used as the process has queues for: lf_streams_effective
  int lf_streams_effective = 0;   // LF streams in use; 0: the rule of lf_group_plan.h LfStreamsForQueues over GPU_MAX_HW_QUEUES as the process has it (3 at 4 queues, 6 at 16)
  int lf_group_max = 4;      // jobs whose SIMT LF kernels may go out as one launch when they are ready together (1: every job its own launch; at most kLfGroupMax)
  int hf_streams = 2;        // HF stages in flight beside the tail (one stream and one coefficient set each, + the set the tail consumes)
  int prepare_threads = 3;   // host threads that each parse + prepare + upload one job at a time
  int parse_threads = 8;     // host threads one job's images are parsed on
  int lane_stride_lf = 8, lane_stride_hf = 1;
  int wide_first = 4;        // LF stages at the start of a cold pipeline that take the one-wavefront-per-stream kernel (shorter latency on an idle GPU)
  int hf_sparse = 0;         // latency mode: small jobs spread their HF group streams over many sparse wavefronts (1 per wavefront up to 8 frames, 4 up to 96)
  int small_job_frames = 0;  // jobs of at most this many frames always take it (latency mode: DeviceScheduler)
  int no_flag_wait = 0;      // the issuing thread never waits for a job's LF stage (placement flags): every IDCT kernel variant is launched instead — latency mode
  int timed = 0;             // bracket the stages with HIP events (CollectTimes)
  // shared coefficient sets / pixel planes are sized for jobs of this shape at creation (0: nothing is reserved; jobs run on arenas of their own until the
  // pipeline is idle, then the shared planes grow to the largest job seen)
  int reserve_frames = 0, reserve_width = 0, reserve_height = 0;
  int reserve_plane_sets = 1;   // 2: frames that take the stage-by-stage filters (anything but gaborish + one EPF pass) need a second set of pixel planes
};

struct PipelineJobResult {
  std::vector<int> status;            // per image: 0 decoded, 1 failed
  std::vector<std::string> error;     // per image: "" or what went wrong
  float end_ms = 0;                   // when the job's last byte had been written / copied, ms after the pipeline's clock was reset
  std::vector<size_t> jpeg_sizes;     // reconstruction jobs: bytes of image i's file (0: none)
};

// flags of a reconstruction job (include/jxl_hip.h JXL_HIP_JPEG_*): the two switches of the batch call
constexpr uint32_t kPipelineJpegDeviceProgressive = 1u, kPipelineJpegHostWriter = 2u;

class Pipeline {
 public:
  Pipeline(int device, const PipelineOptions& opt);
  ~Pipeline();
  // Submits a job of n compressed images, all decoded to `spec`.  Exactly one of device_out / host_out is given: n caller-owned destinations, each at least as large
  // as the image's output in that format (out_capacity[i], when given, is checked).  Host destinations should be pinned (hipHostMalloc / JxlHipHostAlloc) — pageable
  // memory works, slower.  The compressed bytes and the destinations must stay valid until Wait(ticket) returns.  Blocks while `in_flight` jobs are on their way.
  // Returns the job's ticket (>= 0).
  // jpeg_pixels: a libjpeg-exact job (Batch::DecodeJpegPixels as pipeline stages) — every image is decoded to the samples libjpeg gives for the JPEG file it was
  // transcoded from; an image Batch::CanDecodeJpegPixels refuses fails alone with that reason.  `spec` and `each` mean what they mean otherwise; downscale 8 is refused here.
  // spec.jpeg_scale (2, 4, 8: libjpeg's scaled decode) is taken by such a job only, one scale per job; any other job with it is refused.
  // each (optional, n entries): image i is decoded to each[i] instead of `spec` — same format, layout, downscale, jpeg_scale and target size as `spec`; crop, filter and mirror are its own.
  int64_t Submit(const uint8_t* const* datas, const size_t* sizes, int n, const OutputSpec& spec, void* const* device_out, void* const* host_out, const size_t* out_capacity,
                 const OutputSpec* each = nullptr, bool jpeg_pixels = false);
  // A reconstruction job (Batch::ReconstructJpegs as pipeline stages): the original JPEG file of every image, byte for byte.  No output spec and no destinations —
  // nobody can size a JPEG file from its transcode —: the files stay with the pipeline until they are collected.  An image the batch call refuses fails alone with
  // that call's text ("JPEG reconstruction: no jbrd box", ...); a job in which no image can be reconstructed fails as a whole, without touching the GPU.  flags:
  // kPipelineJpegDeviceProgressive / kPipelineJpegHostWriter (Batch::jpeg_device_progressive / jpeg_host_writer; the latter wins); unknown bits refuse the submission.
  // Such jobs mix freely with every other kind over the same coefficient sets and slots.
  int64_t SubmitJpegs(const uint8_t* const* datas, const size_t* sizes, int n, uint32_t flags);
  // Waits like Wait, but keeps the files: JpegStatus / CopyJpeg hand them out until ReleaseJpegs(ticket).  A ticket of another kind is refused (and stays waitable).
  // Wait on a reconstruction ticket gives the statuses and releases the files.  A harvested reconstruction job that nobody waits for holds its files until the
  // bounded history of uncollected jobs drops it (8 x slots + 64 jobs back), and so does one that was waited for and never released.
  void WaitJpegs(int64_t ticket, PipelineJobResult* out);
  int JpegStatus(int64_t ticket, int i, std::string* error);        // 0: image i has a file; 1: *error says why not.  Throws for a ticket that is not held, or no such image
  void CopyJpeg(int64_t ticket, int i, void* dst, size_t capacity);   // throws if the image has no file or the buffer is smaller than it
  void ReleaseJpegs(int64_t ticket);                                // forgets the job and its files (unknown tickets are ignored)
  // Waits until job `ticket` has left the GPU (outputs written, host copies done) and hands out its per-image results; a ticket can be waited for once.
  void Wait(int64_t ticket, PipelineJobResult* out);
  void WaitAll();                                  // every job submitted so far has left the GPU (results stay collectable)
  void ResetClock();                               // end_ms of later jobs counts from here (call on an idle pipeline)
  StageTimes CollectTimes(int* runs);              // per-stage HIP-event sums over all jobs since the last call (options.timed)
  void StageBytes(uint64_t out[6]);                // algorithmic bytes per stage of the job prepared last
  // libjpeg-exact jobs submitted from now on decode crops by region (Batch::jpeg_region): only the groups a crop needs; Info "hf_groups_total" / "hf_groups_decoded" of the job prepared last
  void SetJpegRegion(bool on) { jpeg_region_.store(on); }
  // "lf_group_max" (1 .. kLfGroupMax), "lf_streams_effective" (0: the rule; at most options.lf_streams) for the LF stages issued from now on; "jpeg_region": SetJpegRegion.  false: no such option
  bool SetOption(const std::string& name, int value);
  int64_t Info(const char* name);                  // "lf_groups" / "lf_grouped_jobs" (LF launches and the jobs in them since the last ResetClock), "lf_group_largest", "lf_streams_effective", "device_bytes", "jobs", "shared_big_bytes", "shared_coef_bytes", "private_plane_jobs", "jpeg_pixel_images", "jpeg_pixel_launches" (of the job prepared or finished last), "jpeg_dc_only_images" (of the job finished last), "jpeg_device_images", "jpeg_host_images", "jpeg_device_progressive_images", "jpeg_gather_launches" (of the job finished last; 0 unless it was a reconstruction job), batch infos of the last job ("hf_nonzeros", "lf_simt_frames" ...)
  double prepare_seconds_total() const { return prepare_s_total_; }
  int64_t prepared_jobs() const { return prepared_jobs_; }
  int device() const { return device_; }

 private:
  enum State { kQueued = 0, kPreparing, kPrepared, kFrontIssued, kTailIssued, kHarvested };      // kPrepared: parsed and uploading, waiting for the LF issuer
  // what a job's tail is: the float IDCT, filters and write; the integer IDCT over the HF planes + libjpeg's upsampling and colour conversion (libjpeg-exact pixels);
  // the gather into the JPEG writer's arena + its sizes pass, with the pack pass and the splice at harvest (reconstruction)
  enum Kind { kPlain = 0, kJpegPixels, kJpegFiles };
  struct Job {
    int64_t ticket = 0;
    std::vector<const uint8_t*> datas; std::vector<size_t> sizes;
    std::vector<void*> device_out, host_out; std::vector<size_t> capacity;
    OutputSpec spec;
    std::vector<OutputSpec> each;              // per image, when the job was submitted with specs of its own (empty: `spec` for all)
    Kind kind = kPlain;
    uint32_t jpeg_flags = 0;                   // reconstruction jobs: kPipelineJpeg*
    bool jpeg_region = false;                  // libjpeg-exact jobs: crops are decoded by region (SetJpegRegion as it stood at the submit; Batch::jpeg_region)
    std::vector<vec<uint8_t>> jpeg_files;      // reconstruction jobs, from the harvest on: image i's file (empty: none)
    int64_t jpeg_counts[4] = {0, 0, 0, 0};     // ... device images, host images, device progressive images, gather launches
    bool collected = false;                    // WaitJpegs has returned: the files can be handed out
    std::vector<int> batch_index;              // per image: index in the batch, -1 = failed before it got there
    PipelineJobResult result;
    std::string job_error;                     // the whole job failed (Prepare threw)
    State state = kQueued;
    bool hf_issued = false, waited = false, cold_wide = false;
    bool wide_chain = false;     // one of the chained cold-start jobs
    bool lf_wide = false;        // ... whose LF stage really is the one-wavefront-per-stream launch (set by the LF issuer, which goes through the jobs in ticket order)
    int64_t wide_after = -1;     // cold-start job (one-wavefront-per-stream LF kernel) behind another one: its LF stage waits for that job's, on the device (round 6: four at once took 95-120 ms each, one after the other 55)
    void* done_event = nullptr;                // (timing enabled) recorded behind the job's last copy
  };
  struct Slot {
    std::unique_ptr<Batch> batch;
    void* uploaded = nullptr;                  // behind the job's tables and compressed bytes on the upload stream: what its LF stage waits for
    void *lf_done = nullptr, *front_done = nullptr, *hf_done = nullptr, *idct_done = nullptr, *rest_done = nullptr;
    void* finish_stream = nullptr;             // reconstruction jobs: the stream of FinishJpegWrite at harvest (nothing else queues on it; made when first needed)
    std::mutex mu;                             // harvest of the slot's current job
  };
  void PrepareWorker(int worker);
  void IssuerLoop();
  void LfIssuerLoop();                         // the one thread that enqueues LF stages: in ticket order, jobs that are ready together as one group (Batch::RunLfGroup)
  void IssueLfGroup(const std::vector<std::shared_ptr<Job>>& group, void* stream);
  int LfStreamsInUse() const;
  void PrepareJob(Job* j, int worker);
  void IssueHf(Job* j);
  void IssueTail(Job* j);
  void Harvest(Job* j);                        // waits for the job's completion on the GPU, fills j->result (once)
  Job* FindJob(int64_t ticket);                // (mu_ held)
  int64_t Enqueue(const std::shared_ptr<Job>& job, int n);   // back-pressure, ticket, cold-start chain, history bound, prepare queue
  std::shared_ptr<Job> WaitIssued(int64_t ticket, const char* who, bool jpegs);
  std::shared_ptr<Job> CollectedJpegs(int64_t ticket, int i, const char* who);
  void GrowSharedWhenIdle();                   // (mu_ held, nothing in flight)
  void ReservePlanes(SharedPlanes* sp, size_t bytes);

  const int device_;
  PipelineOptions opt_;
  int nbuf_ = 1, ncoef_ = 2, prio_high_ = 0;
  std::vector<std::unique_ptr<Slot>> slots_;
  SharedPlanes big_;
  std::vector<SharedPlanes> coef_;
  size_t want_big_ = 0, want_coef_ = 0;        // the largest layouts seen: what the shared planes grow to when the pipeline is idle
  void* main_ = nullptr; void* d2h_[2] = {nullptr, nullptr};     // [0]: copies to host + status words of every job, in job order ([1] spare: two streams taking turns measured slower)
  void* upload_ = nullptr;                     // tables and compressed bytes of every job (default priority: not one of the entropy streams' queues)
  std::vector<void*> lf_side_, hf_side_;       // lf_side_: the streams in use (LfStreamsInUse), created when first needed
  std::vector<void*> lf_side_done_;            // per LF stream: recorded behind the last group enqueued on it (nullptr: none yet) — the LF issuer waits for it before the next group
  std::atomic<int> lf_group_max_{4}, lf_streams_effective_{0};
  int64_t lf_groups_ = 0, lf_grouped_jobs_ = 0, lf_group_largest_ = 0;
  void* clock_event_ = nullptr;
  std::mutex mu_;
  std::condition_variable cv_;
  std::map<int64_t, std::shared_ptr<Job>> jobs_;   // submitted, not yet waited for (bounded: old harvested jobs nobody waits for are dropped)
  std::deque<std::shared_ptr<Job>> prep_queue_;
  int64_t next_ticket_ = 0, next_lf_ = 0, next_issue_ = 0, completed_upto_ = 0;   // completed_upto_: every ticket below has state >= kHarvested or has been dropped
  int64_t cold_count_ = 0;
  int64_t private_plane_jobs_ = 0;
  bool shutdown_ = false;
  std::vector<std::thread> workers_;
  std::thread issuer_, lf_issuer_;
  double prepare_s_total_ = 0; int64_t prepared_jobs_ = 0;
  uint64_t last_stage_bytes_[6] = {0, 0, 0, 0, 0, 0};
  std::atomic<bool> jpeg_region_{false};
  std::map<std::string, int64_t> last_info_;
};

// ---- concurrent callers of the libjxl-compatible API (jxl_abi.cc): one shared pipeline per device -----------------------------------------
// A JxlDecoder is used from one thread at a time, different instances concurrently (jpegxl-rs/src/decode.rs:523-532).  Plain one-shot decodes
// (one frame, a caller buffer, no memory manager of the caller's) are handed to the device's scheduler: requests that arrive while earlier ones
// are being prepared ride in one job, so T threads calling decode_with get the batch throughput of the pipeline instead of T serialised decodes.
// Returns 0 and fills dst, or 1 with *error set.
int SchedulerDecode(int device, const uint8_t* data, size_t size, const OutputSpec& spec, void* dst, size_t dst_size, std::string* error);
// statistics of the device's scheduler since the process started: jobs submitted, images decoded (nullptr-safe)
void SchedulerStats(int device, int64_t* jobs, int64_t* images);
void SchedulerNoteDecoder(int delta);   // a JxlDecoder was created (+1) / destroyed (-1): the scheduler sizes its jobs by the decoders that exist (one per calling thread in the reference crate)
void SchedulerShutdown();      // joins the scheduler threads and frees their pipelines (tests; atexit)

}  // namespace jxlhip

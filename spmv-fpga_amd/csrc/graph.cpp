// hipGraph forms of a plan's SpMV: spmv_plan_run_graph's three capture forms (serial chain,
// two-stream DAG, combine riding behind) and the tuner's timed replay.
#include <algorithm>
#include <cstdlib>

#include "spmv_internal.hpp"

using namespace spmvhw;

// Ends the capture on s and instantiates what it recorded into *ge. enqueued: every enqueue
// inside the capture succeeded (else the caller has set the error, and the graph is dropped);
// prefix: what a failed end of capture is reported under.
static int end_capture(hipStream_t s, bool enqueued, const std::string &prefix, hipGraphExec_t *ge)
{
    hipGraph_t g = nullptr;
    const hipError_t ec = hipStreamEndCapture(s, &g);
    if (!enqueued || ec != hipSuccess) {
        if (g)
            (void)hipGraphDestroy(g);
        if (enqueued)
            set_error(prefix + hipGetErrorString(ec));
        return 1;
    }
    const hipError_t ei = hipGraphInstantiate(ge, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    SPMV_TRY(ei);
    return 0;
}

// `iters` serial SpMVs on stream s captured into *ge
static int capture_serial(spmv_plan *p, const ValueType *d_x, ValueType *d_y, int iters, hipStream_t s,
                          hipGraphExec_t *ge)
{
    SPMV_TRY(hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed));
    int rc = 0;
    for (int i = 0; i < iters && !rc; ++i)
        rc = run_impl(p, d_x, d_y, s, false);
    return end_capture(s, !rc, "ec: ", ge);
}

namespace spmvhw {

// ms per SpMV of a layout with scratch x/y, for SPMV_HW_KERNEL=tune: kTuneSteps serial SpMVs
// captured into one hipGraph on a private stream (no host launch gap inside a sample), replayed
// once to warm, then kTuneReps replays each timed with its own event pair; the median replay / steps.
// One timed launch per candidate (round 4) let the timer's noise pick the layout.
constexpr int kTuneSteps = 4, kTuneReps = 7;
int time_layout(spmv_plan &P, const ValueType *d_x, ValueType *d_y, hipStream_t s, double *ms)
{
    SPMV_TRY(hipStreamSynchronize(s));  // the layout was built on s
    struct Res {
        hipStream_t ts = nullptr;
        hipGraphExec_t ge = nullptr;
        hipEvent_t ev[2 * kTuneReps] = {};
        ~Res()
        {
            for (hipEvent_t e : ev)
                if (e)
                    (void)hipEventDestroy(e);
            if (ge)
                (void)hipGraphExecDestroy(ge);
            if (ts)
                (void)hipStreamDestroy(ts);
        }
    } r;
    SPMV_TRY(hipStreamCreateWithFlags(&r.ts, hipStreamNonBlocking));
    for (hipEvent_t &e : r.ev)
        SPMV_TRY(hipEventCreate(&e));
    if (int rc = capture_serial(&P, d_x, d_y, kTuneSteps, r.ts, &r.ge))
        return rc;
    SPMV_TRY(hipGraphLaunch(r.ge, r.ts));  // warm
    for (int k = 0; k < kTuneReps; ++k) {
        SPMV_TRY(hipEventRecord(r.ev[2 * k], r.ts));
        SPMV_TRY(hipGraphLaunch(r.ge, r.ts));
        SPMV_TRY(hipEventRecord(r.ev[2 * k + 1], r.ts));
    }
    SPMV_TRY(hipStreamSynchronize(r.ts));
    std::vector<double> t(kTuneReps);
    for (int k = 0; k < kTuneReps; ++k) {
        float v = 0.f;
        SPMV_TRY(hipEventElapsedTime(&v, r.ev[2 * k], r.ev[2 * k + 1]));
        t[k] = v / kTuneSteps;
    }
    std::nth_element(t.begin(), t.begin() + kTuneReps / 2, t.end());
    *ms = t[kTuneReps / 2];
    return 0;
}

}  // namespace spmvhw

// The "dag" form, for split plans whose sweep launch cannot carry the combine (the behind form
// below measured faster; SPMV_GRAPH_FORM=dag forces this one in the tools build): the combine
// of step k runs on a second capture stream beside the
// sweep of step k + 1, the steps' partial sums alternate between two buffers, and the sweep of
// step k + 2 waits for the combine of step k (its buffer). The combine needs no LDS, so its
// workgroups fit beside the sweep's one 1024-thread workgroup per CU. Every step still computes
// all of y = A x; the y of the last step is complete when the graph ends. Not for the tools
// build's stealing variants (the combine re-arms their counters) or the fused combine.
// (sweep.part: only a split sweep plan has partial sums.)
static bool graph_overlaps(const spmv_plan *p)
{
    return p->sweep.split > 1 && !p->sweep.panel_cnt && p->sweep.part.p && !(p->sweep.variant >= 37 && p->sweep.variant <= 39);
}

static int graph_part2(spmv_plan *p)
{
    if (!p->graph.part2.p)
        SPMV_TRY(p->graph.part2.alloc_bytes(p->sweep.nunits * (uint64_t(p->panels.rmax) + 1) * p->sweep.acc_bytes));
    return 0;
}

static int capture_overlapped(spmv_plan *p, const ValueType *d_x, ValueType *d_y, int iters)
{
    constexpr int R = 2;  // partial buffers (longer rings measured slower)
    if (graph_part2(p))
        return 1;
    if (!p->graph.stream2)
        SPMV_TRY(hipStreamCreateWithFlags(&p->graph.stream2, hipStreamNonBlocking));
    std::vector<hipEvent_t> ev(2 * size_t(iters), nullptr);
    auto destroy = [&] {
        for (hipEvent_t e : ev)
            if (e)
                (void)hipEventDestroy(e);
    };
    for (auto &e : ev)
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
            destroy();
            set_error("spmv_plan_run_graph: hipEventCreate failed");
            return 1;
        }
    hipStream_t a = p->graph.stream, b = p->graph.stream2;
    hipError_t e = hipStreamBeginCapture(a, hipStreamCaptureModeRelaxed);
    for (int k = 0; k < iters && e == hipSuccess; ++k) {
        void *part = k % R ? p->graph.part2.p : p->sweep.part.p;
        if (k >= R)  // this buffer's previous combine is done
            e = hipStreamWaitEvent(a, ev[2 * (k - R) + 1], 0);
        if (e == hipSuccess)
            e = launch_sweep(*p, d_x, d_y, a, false, 1, part);
        if (e == hipSuccess)
            e = hipEventRecord(ev[2 * k], a);
        if (e == hipSuccess)
            e = hipStreamWaitEvent(b, ev[2 * k], 0);
        if (e == hipSuccess)
            e = launch_sweep(*p, d_x, d_y, b, false, 2, part);
        if (e == hipSuccess)
            e = hipEventRecord(ev[2 * k + 1], b);
    }
    if (e == hipSuccess)  // join: the last combine (the combines are in order on b)
        e = hipStreamWaitEvent(a, ev[2 * (iters - 1) + 1], 0);
    const std::string msg = "spmv_plan_run_graph: overlapped capture: ";
    if (e != hipSuccess)
        set_error(msg + hipGetErrorString(e));
    const int rc = end_capture(a, e == hipSuccess, msg, &p->graph.exec);
    destroy();
    return rc;
}

// The "behind" form (default for split plans whose sweep can carry it, sweep_behind_ok): one
// stream, one launch per step, and the combine of step k rides in step k + 1's sweep launch as
// extra blocks that start on the CUs no unit holds and in the sweep's tail (sweep.hip,
// combine_behind); a last k_sweep_combine finishes the last step. Partials alternate between
// sweep.part and graph.part2. No second stream, so no cross-queue hand-off between the steps.
static int capture_behind(spmv_plan *p, const ValueType *d_x, ValueType *d_y, int iters)
{
    if (graph_part2(p))
        return 1;
    if (!p->graph.count) {
        SPMV_TRY(p->graph.count.alloc(2));
        SPMV_TRY(hipMemset(p->graph.count, 0, 2 * sizeof(uint32_t)));
    }
    int ncu = 0;
    SPMV_TRY(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, p->device));
    auto part_of = [&](int k) { return (k & 1) ? p->graph.part2.p : p->sweep.part.p; };
    hipStream_t a = p->graph.stream;
    hipError_t e = hipStreamBeginCapture(a, hipStreamCaptureModeRelaxed);
    for (int k = 0; k < iters && e == hipSuccess; ++k) {
        sweep_behind bh;
        bh.cpart = k ? part_of(k - 1) : nullptr;
        bh.ccount = p->graph.count + (k & 1);
        bh.cnext = p->graph.count + ((k + 1) & 1);
        bh.blocks = (uint32_t)std::max(ncu, 1);
        if (const char *v = ablation_env("SPMV_BEHIND_BLOCKS"))  // tools build: measured settings
            bh.blocks = (uint32_t)std::max(1, atoi(v));
        if (const char *v = ablation_env("SPMV_BEHIND_ROWS"))
            bh.rows_per_thread = (uint32_t)std::max(1, atoi(v) / std::max(1, p->sweep_threads));
        e = launch_sweep(*p, d_x, d_y, a, false, 1, part_of(k), &bh);
    }
    if (e == hipSuccess)  // the last step's combine
        e = launch_sweep(*p, d_x, d_y, a, false, 2, part_of(iters - 1));
    const std::string msg = "spmv_plan_run_graph: behind capture: ";
    if (e != hipSuccess)
        set_error(msg + hipGetErrorString(e));
    return end_capture(a, e == hipSuccess, msg, &p->graph.exec);
}

// the capture form of a run_graph: 0 serial chain, 1 two-stream DAG, 2 behind. The tools build's
// SPMV_GRAPH_FORM=serial|dag|behind forces one (where the plan allows it)
int spmvhw::graph_form(const spmv_plan *p)
{
    const int best = sweep_behind_ok(*p) ? 2 : graph_overlaps(p) ? 1 : 0;
    if (const char *f = ablation_env("SPMV_GRAPH_FORM")) {
        const std::string v(f);
        if (v == "serial")
            return 0;
        if (v == "dag" && best >= 1)
            return 1;
    }
    return best;
}

extern "C" int spmv_plan_run_graph(spmv_plan *p, const ValueType *d_x, ValueType *d_y, int iters, void *stream)
{
    if (!p || iters < 1) {
        set_error("spmv_plan_run_graph: null plan or iters < 1");
        return 1;
    }
    hipStream_t s = (hipStream_t)stream;
    SPMV_TRY(hipSetDevice(p->device));
    if (!p->graph.exec || p->graph.x != d_x || p->graph.y != d_y || p->graph.iters != iters) {
        SPMV_TRY(p->graph.drop_exec());
        if (!p->graph.stream)
            SPMV_TRY(hipStreamCreateWithFlags(&p->graph.stream, hipStreamNonBlocking));
        const int form = iters >= 2 ? graph_form(p) : 0;
        if (form == 2   ? capture_behind(p, d_x, d_y, iters)
            : form == 1 ? capture_overlapped(p, d_x, d_y, iters)
                        : capture_serial(p, d_x, d_y, iters, p->graph.stream, &p->graph.exec))
            return 1;
        p->graph.x = d_x;
        p->graph.y = d_y;
        p->graph.iters = iters;
    }
    hipEvent_t e1 = nullptr;
    if (p->timing.on && timing_begin(p, s, &e1))
        return 1;
    SPMV_TRY(hipGraphLaunch(p->graph.exec, s));
    if (p->timing.on)
        SPMV_TRY(hipEventRecord(e1, s));
    return 0;
}

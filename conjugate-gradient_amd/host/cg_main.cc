// cg_main.cc -- the `cgsolver` command line, both reference forms in one binary.
//
//   cgsolver N OUTFILE [MAXITER]                                  (code/MPI/cg_main.cc:13-69, README.md:63,71)
//   cgsolver FILE.mtx NUM_THREADS BLOCK_WIDTH true|false OUTFILE  (code/CUDA/cg_main.cc:16-63, README.md:98)
//
// If argv[1] parses completely as an integer it is the generator form, otherwise a Matrix-Market path.
// Where the reference took its process count from `srun -n P`, this takes `--gpus P` (or CG_NGPU):
// the binary forks P-1 children BEFORE touching the GPU, one process per MI355X, and the ranks meet over
// pipes (replaces MPI_Init, cg_main.cc:15-20): mailbox IPC handles for the direct-xGMI exchange, or an
// RCCL unique id.
// `--loopback P` runs P logical row blocks on one GPU (CI stand-in for a multi-GPU node).
// `--banded` (NOT a reference mode) holds the matrix as its non-zero diagonals: same recurrence and output, a
// banded mat-vec instead of the dense GEMV; refused if the matrix has more than 64 diagonals.
// `--csr` (NOT a reference mode) holds the matrix as compressed sparse rows (any sparsity pattern): same recurrence and
// output, a CSR mat-vec instead of the dense GEMV.  Not together with --banded.
// `--jacobi` (NOT a reference mode) solves with the Jacobi preconditioner (include/cgx.h cgx_set_preconditioner): same stopping
// test on sqrt(r.r) and the same output, usually fewer iterations on a matrix whose diagonal varies.
// `--jacobi-block B` (implies --jacobi) inverts the B x B diagonal blocks instead of the diagonal entries (B = 1, 2, 4, ..., 256;
// include/cgx.h cgx_set_preconditioner_block).
// `--shifts s0,s1,...` (NOT a reference mode) runs multi-shift CG instead of the plain solve (include/cgx.h cgx_solve_shifted): the
// systems (A + s_j I) x = b for up to 16 shifts s_j >= 0 from one Krylov sequence, one pass over A per iteration.  The timing line
// in OUTFILE is written as ever; one line per shift follows on stdout.  One GPU, dense or --csr, no --jacobi.
// `--minres s0,s1,...` (NOT a reference mode) runs MINRES instead (include/cgx.h cgx_solve_minres): the same systems for up to 16
// shifts of either sign and a symmetric matrix that need not be definite; arguments and output as --shifts.  Not with --shifts.
// `--pivchol K [--pivchol-shift D]` (NOT a reference mode) solves with the rank-K pivoted-Cholesky preconditioner plus shift
// (include/cgx.h CGX_PRECOND_PIVCHOL; D = 0 or absent: the automatic shift): one GPU, dense storage, not with --jacobi.
// `--logdet P[,M]` (NOT a reference mode) estimates log det of the matrix instead of solving (include/cgx.h cgx_trace_slq): stochastic
// Lanczos quadrature with P Rademacher probes (1 ... 256) of M Lanczos steps each (default 100, at most min(n, 1024)).  The timing
// line in OUTFILE is written as ever; one line with the estimate, its standard error and the extreme Ritz values follows on stdout.
// One GPU, dense storage, no preconditioner, not with --shifts; the matrix must be symmetric positive definite.
// `--logdet-pc P[,M]` is the same through the preconditioner that --jacobi or --pivchol K sets (cgx_trace_slq_pc): log det M plus the
// quadrature of M^-1/2 A M^-1/2 with probes of covariance M, M steps each (default 30); the line also prints log det M.
// `--apply NAME[,M[,T]]` (NOT a reference mode) applies a function of the matrix to the source term instead of solving (include/cgx.h
// cgx_apply_function): NAME = sqrt, invsqrt, inv, log or exp (exp(-T A)), M Lanczos steps (default 100, at most min(n, 1024)).  The
// result goes where the solution goes; the timing line in OUTFILE is written as ever and one line with the steps made, the convergence
// indicator and ||x|| follows on stdout.  One GPU, dense storage, no preconditioner, not with --shifts or --logdet.
// `--eigs K[,M[,largest|smallest]]` (NOT a reference mode) computes the K largest (default) or smallest eigenvalues of the matrix instead
// of solving (include/cgx.h cgx_eigenpairs): at most M steps (default 100, at most min(n, 1024)) of Lanczos with full
// reorthogonalisation from the library's start vector (seed 1), tol = 0.  The timing line in OUTFILE is written as ever; one line
// with the steps follows on stdout, then one per eigenvalue with its residual.  One GPU, dense storage, no preconditioner, not
// with --shifts, --logdet or --apply; the matrix must be symmetric.
#include <signal.h>
#include <sys/wait.h>
#include <unistd.h>

#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <iomanip>
#include <iostream>
#include <memory>
#include <mutex>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "cg.hh"

using clk = std::chrono::high_resolution_clock;
using second = std::chrono::duration<double>;

namespace {

bool parse_int(const std::string &s, int *out)
{
    if (s.empty()) return false;
    char *end = nullptr;
    long v = strtol(s.c_str(), &end, 10);
    if (*end != '\0') return false;
    *out = static_cast<int>(v);
    return true;
}

// ---- bounded wire-up ---------------------------------------------------------------------------------------
// Every stage of the multi-GPU wire-up that can block on a peer (the device probe's agreement, the mailbox handle
// exchange, cgx_p2p_import, the self-test, ncclCommInitRank) runs under a deadline.  MPI_Init either returns or the job
// is killed by the scheduler (code/MPI/cg_main.cc:15-20 under srun); here a stage that does not come back makes the rank
// print one line and leave with exit code 1 -- rank 0 first ends and reaps the other ranks -- so that a script like
// experiments/cg_mi355x.run can never hang on a dead peer.  Nothing is retried or restarted in place.
class StageWatchdog {
public:
    StageWatchdog(int rank, const std::vector<pid_t> *kids) : rank_(rank), kids_(kids), thread_([this] { run(); }) {}
    ~StageWatchdog()
    {
        {
            std::lock_guard<std::mutex> lk(m_);
            quit_ = true;
        }
        cv_.notify_all();
        thread_.join();
    }
    void arm(const std::string &stage, double seconds)
    {
        std::lock_guard<std::mutex> lk(m_);
        stage_ = stage;
        seconds_ = seconds;
        deadline_ = std::chrono::steady_clock::now() + std::chrono::duration_cast<std::chrono::steady_clock::duration>(
                                                           std::chrono::duration<double>(seconds));
        armed_ = true;
        cv_.notify_all();
    }
    void disarm()
    {
        std::lock_guard<std::mutex> lk(m_);
        armed_ = false;
        cv_.notify_all();
    }

private:
    void run()
    {
        std::unique_lock<std::mutex> lk(m_);
        while (!quit_) {
            if (!armed_) {
                cv_.wait(lk);
                continue;
            }
            if (cv_.wait_until(lk, deadline_) == std::cv_status::timeout && armed_ && !quit_ &&
                std::chrono::steady_clock::now() >= deadline_) {
                // one write: the ranks expire together and share stderr, piecewise output would interleave
                std::ostringstream msg;
                msg << "cgsolver (rank " << rank_ << "): wire-up stage '" << stage_ << "' did not finish within " << seconds_
                    << " s; giving up\n";
                const std::string text = msg.str();
                if (write(2, text.data(), text.size()) < 0) {}
                if (kids_)   // rank 0: end the other ranks and reap them, so that nothing of the job is left behind
                    for (pid_t k : *kids_) {
                        kill(k, SIGKILL);
                        int st = 0;
                        waitpid(k, &st, 0);
                    }
                _exit(1);
            }
        }
    }
    const int rank_;
    const std::vector<pid_t> *kids_;
    std::mutex m_;
    std::condition_variable cv_;
    bool armed_ = false, quit_ = false;
    std::string stage_;
    double seconds_ = 0;
    std::chrono::steady_clock::time_point deadline_;
    std::thread thread_;
};

int usage(const char *prog)
{
    std::cerr << "Usage: " << prog << " N OUTFILE [MAXITER]            (generated matrix of size N)\n"
              << "       " << prog << " FILE.mtx NUM_THREADS BLOCK_WIDTH true|false OUTFILE\n"
              << "       " << prog << " FILE.mtx OUTFILE [MAXITER]       (matrix file, MPI-form output)\n"
              << "options: --gpus P (or CG_NGPU=P)  one process per MI355X\n"
              << "         --transport auto|p2p|p2p-tag|rccl  exchange: direct xGMI mailboxes (bytes handed over as payload + flag words,\n"
              << "                                  or as tagged words), RCCL; auto = p2p if its self-test passes on every rank, else RCCL\n"
              << "         --wireup-timeout S       seconds any one stage of the multi-GPU wire-up may take (default 120, or\n"
              << "                                  CG_WIREUP_TIMEOUT); a stage that does not come back ends the job with exit code 1\n"
              << "         --loopback P             P logical row blocks on one GPU\n"
              << "         --banded                 opt-in, not in the reference: store the non-zero diagonals only (<= 64)\n"
              << "         --csr                    opt-in, not in the reference: store compressed sparse rows (any pattern;\n"
              << "                                  not together with --banded)\n"
              << "         --jacobi                 opt-in, not in the reference: Jacobi-preconditioned CG (z = D^-1 r; stops on\n"
              << "                                  sqrt(r.r) < tol as without it; dense or CSR storage, per-launch loop)\n"
              << "         --jacobi-block B         implies --jacobi: block Jacobi with the B x B diagonal blocks, B = 1, 2, 4,\n"
              << "                                  ..., 256 (1 = --jacobi; not with --transport p2p)\n"
              << "         --pivchol K              opt-in, not in the reference: CG preconditioned with a rank-K pivoted-Cholesky\n"
              << "                                  factor plus shift (K = 1 ... 256; for dense SPD matrices whose off-diagonal\n"
              << "                                  mass is global; one GPU, dense storage, not with --jacobi)\n"
              << "         --pivchol-shift D        with --pivchol: the shift (default 0 = the mean remaining diagonal)\n"
              << "         --shifts s0,s1,...       opt-in, not in the reference: solve (A + s I) x = b for up to 16 shifts s >= 0 in\n"
              << "                                  one Krylov sequence (multi-shift CG) instead of the plain solve; one GPU, dense\n"
              << "                                  or --csr, not with --jacobi; prints one line per shift\n"
              << "         --minres s0,s1,...       opt-in, not in the reference: the same by MINRES, for shifts of either sign and a\n"
              << "                                  symmetric matrix that need not be definite; one GPU, dense or --csr, not with\n"
              << "                                  --jacobi or --shifts; prints one line per shift\n"
              << "         --logdet P[,M]           opt-in, not in the reference: estimate log det A instead of solving, by stochastic\n"
              << "                                  Lanczos quadrature with P probes (1 ... 256) of M steps (default 100); one GPU,\n"
              << "                                  dense storage, no preconditioner, not with --shifts; prints one line\n"
              << "         --logdet-pc P[,M]        opt-in, not in the reference: --logdet through the preconditioner (needs --jacobi or\n"
              << "                                  --pivchol K): log det M plus P probes (1 ... 256) of M steps (default 30) on\n"
              << "                                  M^-1/2 A M^-1/2; not with --shifts; prints --logdet's line plus log det M\n"
              << "         --apply NAME[,M[,T]]     opt-in, not in the reference: x = f(A) b for the source term b instead of solving, by\n"
              << "                                  M Lanczos steps (default 100); NAME = sqrt, invsqrt, inv, log or exp (exp(-T A),\n"
              << "                                  T >= 0, default 1); one GPU, dense storage, no preconditioner, not with --shifts\n"
              << "                                  or --logdet; prints one line\n"
              << "         --eigs K[,M[,largest|smallest]]  opt-in, not in the reference: the K (1 ... 16) largest (default) or smallest\n"
              << "                                  eigenvalues of the matrix instead of solving, by at most M steps (default 100) of\n"
              << "                                  Lanczos with full reorthogonalisation; one GPU, dense storage, no preconditioner,\n"
              << "                                  not with --shifts, --logdet or --apply; prints one line per eigenvalue\n"
              << "         --stats                  also print iterations/s and K1 GB/s on stderr (event-times every K1:\n"
              << "                                  the seconds in OUTFILE are then a few % higher)" << std::endl;
    return 1;
}

}  // namespace

int main(int argc, char **argv)
{
    // The ranks map each other's mailboxes with hipIpcOpenMemHandle: this host driver only supports dmabuf IPC, which the
    // runtime uses when the legacy mode is switched off.  Must be in the environment before the first HIP call.
    setenv("HSA_ENABLE_IPC_MODE_LEGACY", "0", 0);
    // ---- split options from the reference's positional arguments -------------------------------------
    std::vector<std::string> pos;
    int ngpu = 1, loopback = 0;
    bool stats = false, same_device = false, banded = false, csr = false, jacobi = false;
    std::string transport = "auto";
    std::string test_hang;   // --test-hang-stage
    int jacobi_block = 1;
    int pivchol = 0;             // --pivchol K (0: off)
    double pivchol_shift = 0.0;
    bool have_pivchol_shift = false;
    std::vector<double> shifts;
    bool shifted = false;
    bool minres = false;                                     // --minres: the list is in `shifts`, and `shifted` is set as well
    int logdet_probes = 0, logdet_steps = 100;   // --logdet P[,M] (0 probes: off)
    int logdet_pc_probes = 0, logdet_pc_steps = 30;   // --logdet-pc P[,M] (0 probes: off)
    int apply_fn = -1, apply_steps = 100;        // --apply NAME[,M[,T]] (-1: off)
    double apply_param = 1.0;
    std::string apply_name;
    int eigs_nev = 0, eigs_steps = 100, eigs_which = CGX_EIG_LARGEST;   // --eigs K[,M[,largest|smallest]] (0: off)
    double wireup_timeout = 120.0;
    if (const char *e = getenv("CG_WIREUP_TIMEOUT")) wireup_timeout = atof(e);
    if (const char *e = getenv("CG_NGPU")) ngpu = atoi(e);
    for (int i = 1; i < argc; ++i) {
        std::string a(argv[i]);
        if (a == "--gpus" && i + 1 < argc) ngpu = atoi(argv[++i]);
        else if (a == "--loopback" && i + 1 < argc) loopback = atoi(argv[++i]);
        else if (a == "--stats") stats = true;
        else if (a == "--banded") banded = true;
        else if (a == "--csr") csr = true;
        else if (a == "--jacobi") jacobi = true;
        else if (a == "--jacobi-block" && i + 1 < argc) {
            jacobi = true;
            jacobi_block = atoi(argv[++i]);
        }
        else if (a == "--pivchol" && i + 1 < argc) {
            pivchol = atoi(argv[++i]);
            if (pivchol < 1 || pivchol > CGX_MAX_PRECOND_RANK) {
                std::cerr << argv[0] << ": --pivchol takes a rank 1 ... " << CGX_MAX_PRECOND_RANK << ", not '" << argv[i] << "'\n";
                return usage(argv[0]);
            }
        }
        else if (a == "--pivchol-shift" && i + 1 < argc) {
            char *end = nullptr;
            pivchol_shift = strtod(argv[++i], &end);
            have_pivchol_shift = true;
            if (end == argv[i] || *end != '\0' || !(pivchol_shift >= 0.0) || !(pivchol_shift <= 1.7976931348623157e308)) {
                std::cerr << argv[0] << ": --pivchol-shift takes 0 (automatic) or a positive finite number, not '" << argv[i] << "'\n";
                return usage(argv[0]);
            }
        }
        else if ((a == "--shifts" || a == "--minres") && i + 1 < argc) {
            if (shifted) {
                std::cerr << argv[0] << ": --shifts and --minres are two solvers: give one of them, once\n";
                return usage(argv[0]);
            }
            shifted = true;
            minres = a == "--minres";
            std::stringstream list(argv[++i]);
            std::string item;
            while (std::getline(list, item, ',')) {
                char *end = nullptr;
                const double v = strtod(item.c_str(), &end);
                if (item.empty() || *end != '\0') {
                    std::cerr << argv[0] << ": " << a << " takes a comma-separated list of numbers, not '" << item << "'\n";
                    return usage(argv[0]);
                }
                shifts.push_back(v);
            }
        }
        else if (a == "--logdet" && i + 1 < argc) {
            const std::string arg(argv[++i]);
            const size_t comma = arg.find(',');
            const bool ok = parse_int(arg.substr(0, comma), &logdet_probes) &&
                            (comma == std::string::npos || parse_int(arg.substr(comma + 1), &logdet_steps));
            if (!ok || logdet_probes < 1 || logdet_probes > CGX_MAX_PROBES || logdet_steps < 1 || logdet_steps > CGX_MAX_LANCZOS_STEPS) {
                std::cerr << argv[0] << ": --logdet takes P[,M] with 1 <= P <= " << CGX_MAX_PROBES << " probes and 1 <= M <= "
                          << CGX_MAX_LANCZOS_STEPS << " steps, not '" << arg << "'\n";
                return usage(argv[0]);
            }
        }
        else if (a == "--logdet-pc" && i + 1 < argc) {
            const std::string arg(argv[++i]);
            const size_t comma = arg.find(',');
            const bool ok = parse_int(arg.substr(0, comma), &logdet_pc_probes) &&
                            (comma == std::string::npos || parse_int(arg.substr(comma + 1), &logdet_pc_steps));
            if (!ok || logdet_pc_probes < 1 || logdet_pc_probes > CGX_MAX_PROBES || logdet_pc_steps < 1 ||
                logdet_pc_steps > CGX_MAX_LANCZOS_STEPS) {
                std::cerr << argv[0] << ": --logdet-pc takes P[,M] with 1 <= P <= " << CGX_MAX_PROBES << " probes and 1 <= M <= "
                          << CGX_MAX_LANCZOS_STEPS << " steps, not '" << arg << "'\n";
                return usage(argv[0]);
            }
        }
        else if (a == "--apply" && i + 1 < argc) {
            const std::string arg(argv[++i]);
            std::vector<std::string> part;
            std::stringstream list(arg);
            std::string item;
            while (std::getline(list, item, ',')) part.push_back(item);
            static const char *const names[] = {"sqrt", "invsqrt", "inv", "log", "exp"};   // CGX_FN_SQRT ... CGX_FN_EXP
            bool ok = !part.empty() && part.size() <= 3 && arg.back() != ',';
            if (ok) {
                apply_name = part[0];
                for (int f = 0; f < 5; ++f)
                    if (part[0] == names[f]) apply_fn = f;
                ok = apply_fn >= 0 && (part.size() == 3 ? apply_fn == CGX_FN_EXP : true);
            }
            if (ok && part.size() >= 2) ok = parse_int(part[1], &apply_steps);
            if (ok && part.size() == 3) {
                char *end = nullptr;
                apply_param = strtod(part[2].c_str(), &end);
                ok = !part[2].empty() && *end == '\0' && apply_param >= 0.0 && apply_param <= 1.7976931348623157e308;
            }
            if (!ok || apply_steps < 1 || apply_steps > CGX_MAX_LANCZOS_STEPS) {
                std::cerr << argv[0] << ": --apply takes NAME[,M[,T]] with NAME one of sqrt, invsqrt, inv, log, exp, 1 <= M <= "
                          << CGX_MAX_LANCZOS_STEPS << " steps and, for exp only, a finite T >= 0, not '" << arg << "'\n";
                return usage(argv[0]);
            }
        }
        else if (a == "--eigs" && i + 1 < argc) {
            const std::string arg(argv[++i]);
            std::vector<std::string> part;
            std::stringstream list(arg);
            std::string item;
            while (std::getline(list, item, ',')) part.push_back(item);
            bool ok = !part.empty() && part.size() <= 3 && arg.back() != ',' && parse_int(part[0], &eigs_nev);
            if (ok && part.size() >= 2) ok = parse_int(part[1], &eigs_steps);
            if (ok && part.size() == 3) {
                ok = part[2] == "largest" || part[2] == "smallest";
                eigs_which = part[2] == "smallest" ? CGX_EIG_SMALLEST : CGX_EIG_LARGEST;
            }
            if (!ok || eigs_nev < 1 || eigs_nev > CGX_MAX_EIGENPAIRS || eigs_steps < eigs_nev || eigs_steps > CGX_MAX_LANCZOS_STEPS) {
                std::cerr << argv[0] << ": --eigs takes K[,M[,largest|smallest]] with 1 <= K <= " << CGX_MAX_EIGENPAIRS << " eigenvalues and K <= M <= "
                          << CGX_MAX_LANCZOS_STEPS << " steps, not '" << arg << "'\n";
                eigs_nev = 0;
                return usage(argv[0]);
            }
        }
        else if (a == "--transport" && i + 1 < argc) transport = argv[++i];
        else if (a == "--wireup-timeout" && i + 1 < argc) wireup_timeout = atof(argv[++i]);
        else if (a == "--same-device") same_device = true;   // rehearsal: every rank on device 0 (p2p only)
        else if (a == "--test-hang-stage" && i + 1 < argc) test_hang = argv[++i];   // tests only, see below (not in the usage text)
        else if (a == "--cpu") {
            // SURVEY.md section 8(b) named a --cpu switch for the CPU restatement.  The product has no CPU path by design
            // (a silent fallback would void every parity claim); the restatement is test infrastructure under oracle/.
            std::cerr << argv[0] << ": --cpu is not available: libcgx has no CPU fallback (the CPU restatement of the\n"
                         "reference is the parity oracle under oracle/, used by tests/ and by bench.py's cpu_baseline only)\n";
            return 1;
        }
        else pos.push_back(a);
    }
    if (pos.empty()) return usage(argv[0]);   // cg_main.cc:22-26 (returns 1)
    if (csr && banded) {
        std::cerr << argv[0] << ": --csr and --banded are two storages: give one of them\n";
        return usage(argv[0]);
    }
    if (have_pivchol_shift && !pivchol) {
        std::cerr << argv[0] << ": --pivchol-shift belongs to --pivchol K\n";
        return usage(argv[0]);
    }
    if (pivchol && jacobi) {
        std::cerr << argv[0] << ": --pivchol and --jacobi are two preconditioners: give one of them\n";
        return usage(argv[0]);
    }
    if (logdet_probes && (shifted || jacobi || pivchol)) {
        std::cerr << argv[0] << ": --logdet runs without a preconditioner and not together with --shifts\n";
        return usage(argv[0]);
    }
    if (logdet_pc_probes && (shifted || logdet_probes)) {
        std::cerr << argv[0] << ": --logdet-pc runs not together with --shifts or --logdet\n";
        return usage(argv[0]);
    }
    if (logdet_pc_probes && !(jacobi || pivchol)) {
        std::cerr << argv[0] << ": --logdet-pc needs a preconditioner (--jacobi or --pivchol K); without one --logdet is the call\n";
        return usage(argv[0]);
    }
    if (apply_fn >= 0 && (shifted || jacobi || pivchol || logdet_probes || logdet_pc_probes)) {
        std::cerr << argv[0] << ": --apply runs without a preconditioner and not together with --shifts or --logdet\n";
        return usage(argv[0]);
    }
    if (eigs_nev && (shifted || jacobi || pivchol || logdet_probes || logdet_pc_probes || apply_fn >= 0)) {
        std::cerr << argv[0] << ": --eigs runs without a preconditioner and not together with --shifts, --logdet or --apply\n";
        return usage(argv[0]);
    }
    if (ngpu < 1) ngpu = 1;

    int gen_n = 0;
    const bool gen_form = parse_int(pos[0], &gen_n);
    std::string out_file;
    int max_iter = -1, legacy_nt = 0, legacy_bw = 0;
    bool legacy_t = false, cuda_form = false;
    if (gen_form) {
        if (pos.size() < 2) return usage(argv[0]);
        out_file = pos[1];
        if (pos.size() >= 3) {                // cg_main.cc:37-42
            std::stringstream ss(pos[2]);
            ss >> max_iter;
        }
    } else if (pos.size() >= 5) {
        // CUDA form; the reference reads argv[2..5] unguarded (code/CUDA/cg_main.cc:21-33)
        if (!parse_int(pos[1], &legacy_nt) || !parse_int(pos[2], &legacy_bw)) return usage(argv[0]);
        legacy_t = (pos[3] == "true");
        out_file = pos[4];
        cuda_form = true;
    } else {
        // MPI form with a matrix file: `cgsolver FILE.mtx OUTFILE [MAXITER]`.  The reference's MPI read_matrix
        // never sets the sizes (cg.cc:191-202), so it could not do this; the CSV line is the MPI one.
        if (pos.size() < 2) return usage(argv[0]);
        out_file = pos[1];
        if (pos.size() >= 3) {
            std::stringstream ss(pos[2]);
            ss >> max_iter;
        }
    }

    // ---- one process per GPU: fork before any HIP/RCCL call -------------------------------------------
    // Rank 0 is the hub of a tiny control plane over pipes (what MPI_Init gave the reference): all-gather of a
    // few bytes and an all-min of one int, used to pass the RCCL id / the mailbox IPC handles around.
    int rank = 0;
    std::vector<int> up_rd, down_wr;   // rank 0: one pair per child
    int up_wr = -1, down_rd = -1;      // child: its own pair
    std::vector<pid_t> kids;
    if (ngpu > 1) {
        for (int r = 1; r < ngpu; ++r) {
            int up[2], down[2];
            if (pipe(up) != 0 || pipe(down) != 0) { perror("pipe"); return 1; }
            pid_t pid = fork();
            if (pid < 0) { perror("fork"); return 1; }
            if (pid == 0) {
                rank = r;
                up_wr = up[1];
                down_rd = down[0];
                close(up[0]);
                close(down[1]);
                for (int f : up_rd) close(f);
                for (int f : down_wr) close(f);
                up_rd.clear();
                down_wr.clear();
                kids.clear();
                break;
            }
            kids.push_back(pid);
            up_rd.push_back(up[0]);
            down_wr.push_back(down[1]);
            close(up[1]);
            close(down[0]);
        }
    }
    auto write_all = [](int fd, const void *buf, size_t n) {
        const char *p = static_cast<const char *>(buf);
        while (n) {
            ssize_t k = write(fd, p, n);
            if (k <= 0) throw std::runtime_error("control pipe write failed");
            p += k;
            n -= static_cast<size_t>(k);
        }
    };
    auto read_all = [](int fd, void *buf, size_t n) {
        char *p = static_cast<char *>(buf);
        while (n) {
            ssize_t k = read(fd, p, n);
            if (k <= 0) throw std::runtime_error("control pipe closed (a rank died)");
            p += k;
            n -= static_cast<size_t>(k);
        }
    };
    // every rank contributes `n` bytes; every rank receives all ngpu contributions in rank order
    auto allgather_bytes = [&](const unsigned char *mine, size_t n) {
        std::vector<unsigned char> all(static_cast<size_t>(ngpu) * n);
        if (ngpu == 1) {
            memcpy(all.data(), mine, n);
        } else if (rank == 0) {
            memcpy(all.data(), mine, n);
            for (int r = 1; r < ngpu; ++r) read_all(up_rd[r - 1], all.data() + static_cast<size_t>(r) * n, n);
            for (int r = 1; r < ngpu; ++r) write_all(down_wr[r - 1], all.data(), all.size());
        } else {
            write_all(up_wr, mine, n);
            read_all(down_rd, all.data(), all.size());
        }
        return all;
    };
    auto all_min = [&](int v) {
        unsigned char b = static_cast<unsigned char>(v ? 1 : 0);
        std::vector<unsigned char> all = allgather_bytes(&b, 1);
        for (unsigned char x : all)
            if (!x) return 0;
        return 1;
    };

    int rc = 0;
    try {
        cgx_config cfg;
        cgx_config_init(&cfg);
        cfg.profile_gemv = stats ? 1 : 0;
        cfg.matrix_format = csr ? CGX_MATRIX_CSR : banded ? CGX_MATRIX_BANDED : CGX_MATRIX_DENSE;
        std::unique_ptr<CGSolver> holder;
        if (ngpu > 1) {
            cfg.nranks = ngpu;
            cfg.rank = rank;
            cfg.device = same_device ? 0 : rank;
            // one deadline per stage; the watchdog thread starts here, i.e. after the fork (threads do not survive one)
            StageWatchdog dog(rank, rank == 0 ? &kids : nullptr);
            // --test-hang-stage "<stage>:<rank>" (tests/test_cli_wireup.py): that rank never comes back from that stage.  An
            // explicit argument, not an environment variable: nothing in a user's environment changes what cgsolver does.
            auto stage = [&](const std::string &name, const std::function<void()> &body) {
                struct Armed {          // the deadline ends with the stage, also when its body throws
                    StageWatchdog &d;
                    ~Armed() { d.disarm(); }
                } armed{dog};
                dog.arm(name, wireup_timeout);
                if (!test_hang.empty() && test_hang == name + ":" + std::to_string(rank)) pause();
                body();
            };
            stage("device probe", [&] {
                // every rank must own a usable GPU before any collective wire-up is attempted (a rank that cannot
                // create a context would otherwise leave the others blocked in ncclCommInitRank)
                cgx_config probe;
                cgx_config_init(&probe);
                probe.device = cfg.device;
                cgx_ctx *pc = nullptr;
                const int dev_ok = cgx_create(&pc, &probe) == CGX_OK;
                if (!dev_ok) std::cerr << "cgsolver (rank " << rank << "): " << cgx_last_error(nullptr) << std::endl;
                cgx_destroy(pc);
                if (!all_min(dev_ok)) throw std::runtime_error("--gpus " + std::to_string(ngpu) + ": not every rank has a usable MI355X");
            });
            bool have = false;
            // direct-xGMI mailboxes: create, exchange IPC handles, self-test; all ranks agree on the outcome.  Two forms of
            // the per-iteration exchange, each with its own device code in the self-test: payload + flag words (what auto
            // uses), or tagged 8-byte words (no flags, no fences; on request); RCCL if the mailboxes do not work between these devices.
            std::vector<std::string> forms;
            // auto = the flag form, then RCCL.  The tagged-word form is faster on one GPU (6.9 against 10.2 us per exchange) but
            // rests on an 8-byte half of a 16-byte write-through store arriving untorn over xGMI, which no multi-GPU run has
            // shown yet: it is used on request only (--transport p2p-tag) until one has.
            if (transport == "auto") forms = {"p2p"};
            else if (transport == "p2p-tag" || transport == "p2p") forms = {transport};
            else if (transport != "rccl") throw std::runtime_error("--transport must be auto, p2p-tag, p2p or rccl");
            for (const std::string &form : forms) {
                cfg.comm_mode = CGX_COMM_P2P;
                cfg.p2p_tagged = form == "p2p-tag" ? 1 : 0;
                int ok = 1;
                std::vector<unsigned char> all;
                stage("mailbox allocation (" + form + ")", [&] {
                    unsigned char handle[CGX_IPC_HANDLE_BYTES] = {0};
                    try {
                        holder.reset(new CGSolver(cfg));
                        if (cgx_p2p_export(holder->context(), handle) != CGX_OK) ok = 0;
                    } catch (const std::exception &e) {
                        std::cerr << "cgsolver (rank " << rank << "): " << form << " unavailable: " << e.what() << std::endl;
                        ok = 0;
                    }
                    all = allgather_bytes(handle, CGX_IPC_HANDLE_BYTES);
                    ok = all_min(ok);
                });
                if (ok) {
                    stage("opening the peers' mailboxes (" + form + ")", [&] {
                        if (cgx_p2p_import(holder->context(), all.data()) != CGX_OK) ok = 0;
                        ok = all_min(ok);
                    });
                    if (ok)
                        stage("mailbox self-test (" + form + ")", [&] {
                            int st_ok = 0;
                            if (cgx_p2p_selftest(holder->context(), 32, &st_ok) != CGX_OK) st_ok = 0;
                            have = all_min(st_ok) != 0;
                        });
                }
                if (have) break;
                holder.reset();
                if (rank == 0) std::cerr << "cgsolver: direct peer exchange (" << form << ") unavailable" << std::endl;
            }
            if (!have && (transport == "p2p" || transport == "p2p-tag"))
                throw std::runtime_error("--transport " + transport + ": mailboxes unavailable or self-test failed");
            if (!have && !forms.empty() && rank == 0) std::cerr << "cgsolver: using RCCL" << std::endl;
            cfg.p2p_tagged = 0;
            if (!have) {
                cfg.comm_mode = CGX_COMM_RCCL;
                stage("ncclCommInitRank", [&] {
                    unsigned char uid[CGX_UNIQUE_ID_BYTES] = {0};
                    if (rank == 0 && cgx_comm_unique_id(uid) != CGX_OK)
                        throw std::runtime_error(std::string("cgx_comm_unique_id: ") + cgx_last_error(nullptr));
                    std::vector<unsigned char> all = allgather_bytes(uid, CGX_UNIQUE_ID_BYTES);
                    memcpy(cfg.unique_id, all.data(), CGX_UNIQUE_ID_BYTES);   // rank 0's id
                    holder.reset(new CGSolver(cfg));
                });
            }
        } else {
            if (loopback > 1) {
                cfg.comm_mode = CGX_COMM_LOOPBACK;
                cfg.nranks = loopback;
            }
            holder.reset(new CGSolver(cfg));
        }
        const int psize = cfg.nranks;
        CGSolver &solver = *holder;
        if (jacobi) solver.set_preconditioner(CGX_PRECOND_JACOBI);   // every rank, before the first solve
        if (jacobi_block != 1) solver.set_preconditioner_block(jacobi_block);
        if (pivchol) {
            solver.set_preconditioner(CGX_PRECOND_PIVCHOL);
            solver.set_preconditioner_rank(pivchol);
            solver.set_preconditioner_shift(pivchol_shift);
        }

        if (gen_form) solver.generate_lap2d_matrix(gen_n);   // cg_main.cc:31
        else solver.read_matrix(pos[0]);                     // code/CUDA/cg_main.cc:37
        const int n = solver.n();
        if (max_iter >= 0) solver.set_max_iter(max_iter);
        const double h = 1. / n;                             // cg_main.cc:45-46
        solver.init_source_term(h);
        std::vector<double> x_d(static_cast<size_t>(n), 0.);   // cg_main.cc:49-50

        auto t1 = clk::now();                                // only solve() is timed, cg_main.cc:53-55
        std::vector<double> x_shifted;                       // --shifts: one solution per shift
        double slq[4] = {0, 0, 0, 0};                        // --logdet: estimate, standard error, smallest / largest Ritz value
        double slq_pc = 0;                                   // --logdet-pc: log det of the preconditioner
        int apply_done = 0;                                  // --apply: the steps made and the convergence indicator
        double apply_change = 0;
        double eig_val[CGX_MAX_EIGENPAIRS] = {0}, eig_res[CGX_MAX_EIGENPAIRS] = {0}, eig_est[CGX_MAX_EIGENPAIRS] = {0};   // --eigs
        int eig_done = 0, eig_found = 0;
        if (logdet_probes) {
            if (cgx_trace_slq(solver.context(), CGX_SLQ_LOG, logdet_probes, logdet_steps, 1ull, nullptr, 0, &slq[0], &slq[1], nullptr,
                              &slq[2]) != CGX_OK)
                throw std::runtime_error(std::string("--logdet: ") + cgx_last_error(solver.context()));
        }
        else if (logdet_pc_probes) {
            if (cgx_trace_slq_pc(solver.context(), CGX_SLQ_LOG, logdet_pc_probes, logdet_pc_steps, 1ull, nullptr, 0, &slq[0], &slq[1], nullptr,
                                 &slq[2], &slq_pc) != CGX_OK)
                throw std::runtime_error(std::string("--logdet-pc: ") + cgx_last_error(solver.context()));
        }
        else if (apply_fn >= 0) {
            std::vector<double> b(static_cast<size_t>(n), 0.);
            if (cgx_probe_get_source_term(solver.context(), 0, b.data()) != CGX_OK ||
                cgx_apply_function(solver.context(), apply_fn, apply_param, 1, apply_steps, b.data(), n, x_d.data(), n, &apply_done, &apply_change,
                                   nullptr) != CGX_OK)
                throw std::runtime_error(std::string("--apply: ") + cgx_last_error(solver.context()));
        }
        else if (eigs_nev) {
            if (cgx_eigenpairs(solver.context(), eigs_which, eigs_nev, eigs_steps, 0.0, nullptr, 1ull, eig_val, nullptr, 0, eig_res, eig_est,
                               &eig_done, &eig_found) != CGX_OK)
                throw std::runtime_error(std::string("--eigs: ") + cgx_last_error(solver.context()));
        }
        else if (minres) solver.solve_minres(shifts, x_shifted);
        else if (shifted) solver.solve_shifted(shifts, x_shifted);
        else if (cuda_form) solver.solve(x_d.data(), legacy_nt, legacy_bw, legacy_t);
        else solver.solve(x_d);
        second elapsed = clk::now() - t1;

        if (rank == 0) {
            std::ofstream outfile(out_file.c_str(), std::ios_base::app);
            if (!cuda_form) {
                outfile << n << "," << psize << "," << elapsed.count() << std::endl;   // cg_main.cc:62
            } else {
                std::cout << "Time for CG (dense solver)  = " << elapsed.count() << " [s]\n";   // code/CUDA/cg_main.cc:54
                outfile << legacy_nt << "," << legacy_bw << "," << elapsed.count() << std::endl;   // :59
            }
            if (logdet_probes)
                std::cout << "\t[LOGDET] probes = " << logdet_probes << ", steps = " << logdet_steps << ", log det A = " << std::setprecision(12)
                          << slq[0] << ", standard error = " << std::setprecision(6) << slq[1] << ", Ritz values in [" << slq[2] << ", "
                          << slq[3] << "]" << std::endl;
            if (logdet_pc_probes)
                std::cout << "\t[LOGDET] probes = " << logdet_pc_probes << ", steps = " << logdet_pc_steps << ", log det A = "
                          << std::setprecision(12) << slq[0] << ", standard error = " << std::setprecision(6) << slq[1]
                          << ", Ritz values in [" << slq[2] << ", " << slq[3] << "], log det M = " << std::setprecision(12) << slq_pc
                          << std::setprecision(6) << std::endl;
            if (apply_fn >= 0) {
                double xx = 0.0;
                for (double v : x_d) xx += v * v;
                std::cout << "\t[APPLY] fn = " << apply_name << ", steps = " << apply_steps << ", steps_done = " << apply_done
                          << ", change = " << std::setprecision(12) << apply_change << ", ||x|| = " << std::sqrt(xx) << std::setprecision(6)
                          << std::endl;
            }
            if (eigs_nev) {
                std::cout << "\t[EIGS] which = " << (eigs_which == CGX_EIG_SMALLEST ? "smallest" : "largest") << ", nev = " << eigs_nev
                          << ", steps = " << eigs_steps << ", steps_done = " << eig_done << ", nfound = " << eig_found << std::endl;
                for (int j = 0; j < eig_found; ++j)
                    std::cout << "\t[EIG " << j << "] value = " << std::setprecision(17) << eig_val[j] << ", residual = " << std::setprecision(12)
                              << eig_res[j] << ", estimate = " << eig_est[j] << std::setprecision(6) << std::endl;
            }
            if (shifted) {
                const std::vector<cgx_result> &sr = solver.shift_results();
                for (size_t j = 0; j < sr.size(); ++j)
                    std::cout << "\t[SHIFT " << shifts[j] << "] iterations = " << sr[j].iterations << ", converged = " << sr[j].converged
                              << ", residual = " << std::scientific << (minres ? sr[j].residual_last : sr[j].residual_prev) << ", ||(A + sI)x - b||/||b|| = "
                              << sr[j].rel_residual << std::defaultfloat << std::endl;
            }
            if (stats) {
                const cgx_result &r = solver.last_result();
                const int it = r.iterations + (r.converged ? 1 : 0);   // loop bodies executed
                int plan[CGX_GEMV_PLAN_INTS] = {0};
                (void)cgx_get_gemv_plan(solver.context(), 0, plan);     // variant 4 / 5: the loop ran as one persistent kernel
                long long rec[CGX_RESIDENT_RECORD_INTS] = {0};
                (void)cgx_get_resident_record(solver.context(), rec);
                const bool persistent = plan[0] == 4 || plan[0] == 5;
                std::cerr << "cgsolver stats: n=" << n << " gpus=" << psize << " loop_bodies=" << it
                          << " loop_s=" << r.seconds_loop << " iterations_per_s=" << (r.seconds_loop > 0 ? it / r.seconds_loop : 0.)
                          << " format=" << (csr ? "csr" : banded ? "banded" : "dense");
                if (csr) {
                    long long nnz = 0;
                    (void)cgx_get_matrix_nnz(solver.context(), 0, &nnz);
                    std::cerr << " nnz=" << nnz;
                }
                std::cerr
                          << " loop=" << (plan[0] == 4 ? "resident-kernel" : plan[0] == 5 ? "streaming-persistent-kernel" : "per-launch");
                if (persistent) {
                    // no K1 launches to time: the whole loop against the algorithmic bytes of its GEMVs, and what its waits cost
                    // (cgx_get_resident_record; ticks of 10 ns)
                    std::cerr << " gemv_ms_avg=n/a loop_GBps=" << (r.seconds_loop > 0 ? it * r.gemv_bytes / r.seconds_loop / 1e9 : 0.)
                              << " loop_hbm_roofline_frac=" << (r.seconds_loop > 0 ? it * r.gemv_bytes / r.seconds_loop / 8.0e12 : 0.)
                              << " launches=" << rec[3] << " watch_repeats=" << rec[1] << " gather_repeats=" << rec[2]
                              << " first_wait_us=" << rec[4] / 100.0 << " longest_later_wait_us=" << rec[5] / 100.0
                              << " first_wait_us_any_wg=" << rec[6] / 100.0 << " longest_later_wait_us_any_wg=" << rec[7] / 100.0;
                } else {
                    std::cerr << " gemv_ms_avg=" << r.gemv_ms_avg
                              << " gemv_GBps_per_gpu=" << (r.gemv_ms_avg > 0 ? r.gemv_bytes / (r.gemv_ms_avg * 1e-3) / 1e9 : 0.)
                              << " hbm_roofline_frac=" << (r.gemv_ms_avg > 0 ? r.gemv_bytes / (r.gemv_ms_avg * 1e-3) / 8.0e12 : 0.);
                }
                std::cerr << " persistent_launches_redone_per_launch=" << rec[8];
                if (jacobi) std::cerr << " precond=jacobi";   // only when set: the plain line stays as it was
                if (jacobi_block != 1) std::cerr << " block=" << jacobi_block;
                if (pivchol) {
                    double set = 0, used = 0;
                    (void)cgx_get_preconditioner_shift(solver.context(), &set, &used);
                    std::cerr << " precond=pivchol rank=" << pivchol << " shift=" << used << " converged=" << r.converged;
                }
                std::cerr << std::endl;
            }
        }
    } catch (const std::exception &e) {
        // one write per message: the ranks share stderr and tend to fail together
        const std::string msg = "cgsolver (rank " + std::to_string(rank) + "): " + e.what() + "\n";
        if (write(2, msg.data(), msg.size()) < 0) {}
        rc = 1;
    }

    // rank 0 reaps the other ranks; if it failed itself they may be blocked on it (a pipe read, a collective): end them
    for (pid_t k : kids) {
        if (rc != 0) kill(k, SIGTERM);
        int st = 0;
        waitpid(k, &st, 0);
        if (!WIFEXITED(st) || WEXITSTATUS(st) != 0) rc = 1;
    }
    return rc;
}

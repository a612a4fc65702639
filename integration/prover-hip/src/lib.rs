//! `prove_cairo_m_hip` — the MI355X twin of `cairo_m_prover::prover::prove_cairo_m::<Blake2sMerkleChannel>`
//! (crates/prover/src/prover.rs:23-147): same arguments, same result type, same error type.  The whole Stwo path runs in
//! libcairom_hip.so (hand-written gfx950 kernels); this crate only flattens `ProverInput` into the C ABI
//! (include/cairom_hip.h `cm_prover_input`) and deserialises the returned `Proof<Blake2sMerkleHasher>` JSON.
//!
//! Shipped as source: the HIP repository's build image has no Rust toolchain, so this file has never been compiled there.
//! The two data-layout contracts it relies on are tested on the C side: the proof JSON has exactly the serde shape of
//! `Proof<H>` (tests/test_proof_json.py, schema extracted from this reference's structs) and `cm_prover_input` is what the
//! HIP prover is tested against (tests/test_gpu_prove.py).
pub mod backend;
pub mod ffi;
pub mod flat;

use std::ffi::CStr;
use std::sync::Once;

use cairo_m_prover::Proof;
use cairo_m_prover::adapter::ProverInput;
use cairo_m_prover::errors::{ProvingError, VerificationError};
use cairo_m_prover::prover_config::REGULAR_96_BITS;
use stwo_prover::core::pcs::PcsConfig;
use stwo_prover::core::prover::{ProvingError as StwoProvingError, VerificationError as StwoVerificationError};
use stwo_prover::core::vcs::blake2_merkle::Blake2sMerkleHasher;

use ffi::*;
use flat::{Flat, MemoryOrder};

/// Opcode groups of `define_opcodes!` (crates/prover/src/components/opcodes/mod.rs:223-268), in macro order: component k
/// of the HIP library = group k; inside a group the bundles of the listed opcodes are concatenated in this order, exactly
/// as `opcodes::Claim::write_trace` does (opcodes/mod.rs:51-58).
pub(crate) const OPCODE_GROUPS: [&[u32]; CM_N_OPCODE_COMPONENTS] = {
    use cairo_m_common::instruction::*;
    [
        &[ASSERT_EQ_FP_IMM],
        &[CALL_ABS_IMM],
        &[JMP_ABS_IMM, JMP_REL_IMM],
        &[JNZ_FP_IMM],
        &[RET],
        &[STORE_IMM],
        &[STORE_ADD_FP_FP, STORE_SUB_FP_FP, STORE_MUL_FP_FP, STORE_DIV_FP_FP],
        &[STORE_ADD_FP_IMM, STORE_MUL_FP_IMM],
        &[STORE_DOUBLE_DEREF_FP, STORE_TO_DOUBLE_DEREF_FP_IMM],
        &[STORE_DOUBLE_DEREF_FP_FP, STORE_TO_DOUBLE_DEREF_FP_FP],
        &[STORE_FRAME_POINTER],
        &[U32_STORE_IMM],
        &[U32_STORE_ADD_FP_IMM],
        &[U32_STORE_MUL_FP_IMM],
        &[U32_STORE_DIV_REM_FP_IMM],
        &[U32_STORE_EQ_FP_FP],
        &[U32_STORE_EQ_FP_IMM],
        &[U32_STORE_LT_FP_IMM],
        &[U32_STORE_LT_FP_FP],
        &[U32_STORE_ADD_FP_FP],
        &[U32_STORE_SUB_FP_FP],
        &[U32_STORE_MUL_FP_FP],
        &[U32_STORE_DIV_REM_FP_FP],
        &[U32_STORE_AND_FP_FP, U32_STORE_OR_FP_FP, U32_STORE_XOR_FP_FP],
        &[U32_STORE_AND_FP_IMM, U32_STORE_OR_FP_IMM, U32_STORE_XOR_FP_IMM],
        &[STORE_LE_FP_IMM],
    ]
};

pub(crate) fn last_error() -> String {
    let mut buf = vec![0i8; 2048];
    unsafe {
        cm_last_error(buf.as_mut_ptr(), buf.len());
        CStr::from_ptr(buf.as_ptr()).to_string_lossy().into_owned()
    }
}

/// Selects the GPU once per process (one process per GPU; `CAIROM_HIP_DEVICE` or LOCAL_RANK picks the device).
pub(crate) fn ensure_init() {
    static INIT: Once = Once::new();
    INIT.call_once(|| {
        let dev = std::env::var("CAIROM_HIP_DEVICE")
            .or_else(|_| std::env::var("LOCAL_RANK"))
            .ok()
            .and_then(|s| s.parse().ok())
            .unwrap_or(0);
        let rc = unsafe { cm_init(dev) };
        assert!(rc == 0, "cm_init({dev}) failed: {}", last_error());
    });
}

fn pcs(c: &PcsConfig) -> cm_pcs_config {
    cm_pcs_config {
        pow_bits: c.pow_bits,
        log_blowup_factor: c.fri_config.log_blowup_factor,
        log_last_layer_degree_bound: c.fri_config.log_last_layer_degree_bound,
        n_queries: c.fri_config.n_queries as u32,
    }
}

struct ProofHandle(*mut cm_proof);
impl Drop for ProofHandle {
    fn drop(&mut self) {
        unsafe { cm_proof_free(self.0) };
    }
}

/// Twin of `prove_cairo_m::<Blake2sMerkleChannel>` (crates/prover/src/prover.rs:23-29).  `input` is consumed in place the
/// same way (bundle vectors drained).  Status 10 of the library = the one Stwo error the reference surfaces
/// (`ConstraintsNotSatisfied`, errors.rs:14-18); any other failure is a bug or a device error and panics, like the
/// `unwrap`/`expect`s of the reference path do.
pub fn prove_cairo_m_hip(input: &mut ProverInput, pcs_config: Option<PcsConfig>) -> Result<Proof<Blake2sMerkleHasher>, ProvingError> {
    ensure_init();
    let cfg = pcs(&pcs_config.unwrap_or(REGULAR_96_BITS));
    // ascending addresses: the reference iterates a HashMap here (components/memory.rs:105-109), i.e. an unspecified order
    let flat = Flat::new(input, MemoryOrder::AscendingAddress);
    let view = flat.view();
    let mut out: *mut cm_proof = std::ptr::null_mut();
    let rc = unsafe { cm_prove_segment(&view, &cfg, &mut out) };
    match rc {
        0 => {}
        10 => return Err(ProvingError::Stwo(StwoProvingError::ConstraintsNotSatisfied)),
        _ => panic!("libcairom_hip: status {rc}: {}", last_error()),
    }
    let handle = ProofHandle(out);
    let (mut ptr, mut len) = (std::ptr::null(), 0usize);
    let rc = unsafe { cm_proof_json(handle.0, &mut ptr, &mut len) };
    assert!(rc == 0, "cm_proof_json: {}", last_error());
    let json = unsafe { std::slice::from_raw_parts(ptr as *const u8, len) };
    // serde layout of `Proof<H>` (lib.rs:61-73), the text `sonic_rs::to_string(&proof)` would produce (main.rs:86-91)
    let proof: Proof<Blake2sMerkleHasher> = sonic_rs::from_slice(json).expect("libcairom_hip returned a malformed Proof JSON");
    Ok(proof)
}

/// Streaming form for a service that proves the continuation segments of a run (crates/runner/src/vm/mod.rs:184-240 cuts them,
/// crates/prover/tests/prover.rs:203-243 proves them one by one): `cm_prove_many_host` uploads segment k + 1 on the calling
/// thread while up to `inflight` library threads prove the segments before it, so the 6 ms PCIe copy of a 2^22-step segment hides
/// under the 10 ms proof of its predecessor.  Proofs come back in input order; the first failing segment is reported
/// (`ConstraintsNotSatisfied` for status 10) after the others have been proved.
pub fn prove_segments_hip(
    inputs: &mut [ProverInput],
    pcs_config: Option<PcsConfig>,
    inflight: u32,
) -> Result<Vec<Proof<Blake2sMerkleHasher>>, ProvingError> {
    ensure_init();
    let cfg = pcs(&pcs_config.unwrap_or(REGULAR_96_BITS));
    let flats: Vec<Flat> = inputs.iter_mut().map(|i| Flat::new(i, MemoryOrder::AscendingAddress)).collect();
    let views: Vec<_> = flats.iter().map(|f| f.view()).collect();
    let ptrs: Vec<*const cm_prover_input> = views.iter().map(|v| v as *const cm_prover_input).collect();
    let mut outs: Vec<*mut cm_proof> = vec![std::ptr::null_mut(); inputs.len()];
    let rc = unsafe { cm_prove_many_host(ptrs.as_ptr(), ptrs.len() as u32, &cfg, inflight, outs.as_mut_ptr()) };
    let handles: Vec<ProofHandle> = outs.into_iter().filter(|p| !p.is_null()).map(ProofHandle).collect();   // freed on drop
    match rc {
        0 => {}
        10 => return Err(ProvingError::Stwo(StwoProvingError::ConstraintsNotSatisfied)),
        _ => panic!("libcairom_hip: status {rc}: {}", last_error()),
    }
    handles
        .iter()
        .map(|h| {
            let (mut ptr, mut len) = (std::ptr::null(), 0usize);
            let rc = unsafe { cm_proof_json(h.0, &mut ptr, &mut len) };
            assert!(rc == 0, "cm_proof_json: {}", last_error());
            let json = unsafe { std::slice::from_raw_parts(ptr as *const u8, len) };
            Ok(sonic_rs::from_slice(json).expect("libcairom_hip returned a malformed Proof JSON"))
        })
        .collect()
}

/// One segment of a run in the runner's own terms: `(pc, fp)` pairs, the memory log (five words per access) and the lengths of
/// the runner's locals / heap vectors when the segment ends.
pub struct RunSegment<'a> {
    pub trace: &'a [u32],
    pub memory_trace: &'a [u32],
    pub n_memory_end: u64,
    pub n_heap_end: u64,
}

/// A whole run (`cm_prove_run`, header revision 10): the memory at the start of the run is uploaded once and carried on the
/// device; every segment brings only its trace and its log.  `ranges` = program, input, output `[start, end)`.  The proofs come
/// back in segment order and chain: `cm_verify_run` has checked that each starts where its predecessor stopped.
pub fn prove_run_hip(
    initial_memory: &[u32],
    initial_heap: &[u32],
    ranges: [u32; 6],
    segments: &[RunSegment],
    pcs_config: Option<PcsConfig>,
    inflight: u32,
) -> Result<Vec<Proof<Blake2sMerkleHasher>>, ProvingError> {
    ensure_init();
    let cfg = pcs(&pcs_config.unwrap_or(REGULAR_96_BITS));
    let mut run: *mut cm_run = std::ptr::null_mut();
    let rc = unsafe {
        cm_run_begin(initial_memory.as_ptr(), (initial_memory.len() / 4) as u64, initial_heap.as_ptr(), (initial_heap.len() / 4) as u64, ranges.as_ptr(), &mut run)
    };
    assert!(rc == 0, "cm_run_begin: {}", last_error());
    let views: Vec<cm_run_segment> = segments
        .iter()
        .map(|s| cm_run_segment {
            trace: s.trace.as_ptr(),
            n_trace: (s.trace.len() / 2) as u64,
            memory_trace: s.memory_trace.as_ptr(),
            n_memory_trace: (s.memory_trace.len() / 5) as u64,
            n_memory_end: s.n_memory_end,
            n_heap_end: s.n_heap_end,
        })
        .collect();
    let ptrs: Vec<*const cm_run_segment> = views.iter().map(|v| v as *const cm_run_segment).collect();
    let mut outs: Vec<*mut cm_proof> = vec![std::ptr::null_mut(); segments.len()];
    let rc = unsafe { cm_prove_run(run, ptrs.as_ptr(), ptrs.len() as u32, &cfg, inflight, outs.as_mut_ptr()) };
    unsafe { cm_run_free(run) };
    let handles: Vec<ProofHandle> = outs.into_iter().filter(|p| !p.is_null()).map(ProofHandle).collect();   // freed on drop
    match rc {
        0 => {}
        10 => return Err(ProvingError::Stwo(StwoProvingError::ConstraintsNotSatisfied)),
        _ => panic!("libcairom_hip: status {rc}: {}", last_error()),
    }
    let raw: Vec<*const cm_proof> = handles.iter().map(|h| h.0 as *const cm_proof).collect();
    let rc = unsafe { cm_verify_run(raw.as_ptr(), raw.len() as u32, &cfg) };
    assert!(rc == 0, "cm_verify_run: {}", last_error());
    handles
        .iter()
        .map(|h| {
            let (mut ptr, mut len) = (std::ptr::null(), 0usize);
            let rc = unsafe { cm_proof_json(h.0, &mut ptr, &mut len) };
            assert!(rc == 0, "cm_proof_json: {}", last_error());
            let json = unsafe { std::slice::from_raw_parts(ptr as *const u8, len) };
            Ok(sonic_rs::from_slice(json).expect("libcairom_hip returned a malformed Proof JSON"))
        })
        .collect()
}

/// `verify_cairo_m::<Blake2sMerkleChannel>` stays the reference's own function: the value returned above is an ordinary
/// `Proof<Blake2sMerkleHasher>`.  This helper is the library-side verifier (host code, no GPU) for callers that want the
/// check without Stwo: same acceptance conditions, error mapped onto the reference's enum.
pub fn verify_words_hip(proof: &ProofHandleRef, pcs_config: Option<PcsConfig>) -> Result<(), VerificationError> {
    let cfg = pcs(&pcs_config.unwrap_or(REGULAR_96_BITS));
    let rc = unsafe { cm_verify_proof(proof.0, &cfg) };
    match rc {
        0 => Ok(()),
        _ if last_error().contains("InvalidLogupSum") => Err(VerificationError::InvalidLogupSum),
        _ if last_error().contains("ProofOfWork") => Err(VerificationError::Stwo(StwoVerificationError::ProofOfWork)),
        _ if last_error().contains("OodsNotMatching") => Err(VerificationError::Stwo(StwoVerificationError::OodsNotMatching)),
        _ => Err(VerificationError::Stwo(StwoVerificationError::InvalidStructure(last_error()))),
    }
}
/// `cm_verify_many`: the same verdicts for a whole batch of library proofs, computed on the GPU in one call (the host plans, the
/// device hashes every decommitment path and folds the FRI layers).  One entry per proof, in order; the error carries the words
/// `cm_verify_proof` would have left for that proof.  Panics when the batch cannot be run at all (no GPU, null proof).
pub fn verify_cairo_m_many(proofs: &[ProofHandleRef], pcs_config: Option<PcsConfig>) -> Vec<Result<(), VerificationError>> {
    verify_many_with_flags(proofs, pcs_config, 0)
}
/// `cm_verify_many_ex` with `CM_VERIFY_ARITH_ON_DEVICE`: as `verify_cairo_m_many`, with the public LogUp sum and the OODS
/// composition check of every proof decided on the GPU as well (worth it for proofs with large public programs).  Same verdicts.
pub fn verify_cairo_m_many_arith_on_device(proofs: &[ProofHandleRef], pcs_config: Option<PcsConfig>) -> Vec<Result<(), VerificationError>> {
    verify_many_with_flags(proofs, pcs_config, CM_VERIFY_ARITH_ON_DEVICE)
}
fn verify_many_with_flags(proofs: &[ProofHandleRef], pcs_config: Option<PcsConfig>, flags: u32) -> Vec<Result<(), VerificationError>> {
    ensure_init();
    let cfg = pcs(&pcs_config.unwrap_or(REGULAR_96_BITS));
    let raw: Vec<*const cm_proof> = proofs.iter().map(|p| p.0).collect();
    let mut results = vec![cm_verify_result { status: 0, check: 0, message: [0; 160] }; raw.len()];
    let rc = unsafe { cm_verify_many_ex(raw.as_ptr(), raw.len() as u32, &cfg, flags, results.as_mut_ptr(), 0) };
    assert!(rc == 0 || rc == 11, "cm_verify_many: status {rc}: {}", last_error());
    results
        .iter()
        .map(|r| {
            if r.status == 0 {
                return Ok(());
            }
            let msg = unsafe { std::ffi::CStr::from_ptr(r.message.as_ptr()) }.to_string_lossy().into_owned();
            Err(match r.check {
                3 => VerificationError::InvalidLogupSum,
                2 | 6 => VerificationError::Stwo(StwoVerificationError::ProofOfWork),
                4 => VerificationError::Stwo(StwoVerificationError::OodsNotMatching),
                _ => VerificationError::Stwo(StwoVerificationError::InvalidStructure(msg)),
            })
        })
        .collect()
}
/// Borrowed library proof object (e.g. kept by a caller that proves many segments and verifies them later).
pub struct ProofHandleRef(pub *const cm_proof);
impl ProofHandleRef {
    /// `Proof::program_id()` of the reference for a library proof (`cm_proof_program_id`, host code, no GPU): the Poseidon2 root of
    /// the partial memory tree that holds only the proof's public program cells.  Where the reference panics (an absent program
    /// entry, no program at all) this returns the library's words instead.
    pub fn program_id(&self) -> Result<u32, String> {
        let mut id = 0u32;
        let rc = unsafe { cm_proof_program_id(self.0, &mut id) };
        if rc == 0 {
            Ok(id)
        } else {
            Err(last_error())
        }
    }
}
/// `cm_proofs_program_ids`: the ids of a whole batch of library proofs, hashed on the GPU in one call (one upload, two launches,
/// one download).  One entry per proof, in order; `Err` for a proof whose program has no id.  Panics when the batch cannot be run
/// at all (no GPU, no proofs).
pub fn program_ids(proofs: &[ProofHandleRef]) -> Vec<Result<u32, String>> {
    ensure_init();
    let raw: Vec<*const cm_proof> = proofs.iter().map(|p| p.0).collect();
    let mut ids = vec![0u32; raw.len()];
    let mut status = vec![0i32; raw.len()];
    let rc = unsafe { cm_proofs_program_ids(raw.as_ptr(), raw.len() as u32, ids.as_mut_ptr(), status.as_mut_ptr(), 0) };
    let words = last_error();
    assert!(rc == 0 || (rc == 1 && words.starts_with("item ")), "cm_proofs_program_ids: status {rc}: {words}");
    ids.iter()
        .zip(status.iter())
        .enumerate()
        .map(|(i, (id, st))| {
            if *st == 0 {
                Ok(*id)
            } else {
                Err(format!("item {i}: the program has no id ({words})"))
            }
        })
        .collect()
}
/// `cm_run_statement_of`: what a chain of library proofs states.  The chain check of `cm_verify_run` (`device`: of
/// `cm_verify_run_device`) comes first, then every segment must carry segment 0's program, then the program's id is hashed once
/// (on the GPU when `device`) and compared with `expected_program_id` when that is given.  `Err` carries the library's status and
/// words: 11 for a chain that does not verify, does not link, changes its program or is about another program.
pub fn run_statement(
    proofs: &[ProofHandleRef],
    pcs_config: Option<PcsConfig>,
    expected_program_id: Option<u32>,
    device: bool,
) -> Result<cm_run_statement, (i32, String)> {
    if device {
        ensure_init();
    }
    let cfg = pcs(&pcs_config.unwrap_or(REGULAR_96_BITS));
    let raw: Vec<*const cm_proof> = proofs.iter().map(|p| p.0).collect();
    let mut out = cm_run_statement { struct_size: std::mem::size_of::<cm_run_statement>() as u32, ..Default::default() };
    let want = expected_program_id.as_ref().map_or(std::ptr::null(), |x| x as *const u32);
    let rc = unsafe { cm_run_statement_of(raw.as_ptr(), raw.len() as u32, &cfg, want, device as u32, &mut out) };
    if rc == 0 {
        Ok(out)
    } else {
        Err((rc, last_error()))
    }
}

/// Why `assert_constraints` rejected an input: the library's whole report (per-component failing rows, lowest failing
/// (row, constraint), claimed sums, per-relation sums, the relations used) and its one-line verdict.
#[derive(Clone)]
pub struct ConstraintFailure {
    pub report: Box<cm_check_report>,
    pub message: String,
}
impl std::fmt::Debug for ConstraintFailure {
    fn fmt(&self, f: &mut std::fmt::Formatter<'_>) -> std::fmt::Result {
        write!(f, "ConstraintFailure(status {}: {})", self.report.status, self.message)
    }
}
impl ConstraintFailure {
    /// names of the relations whose sums over all components and the public data do not cancel (status 3 names them too)
    pub fn unbalanced_relations(&self) -> Vec<&'static str> {
        const NAMES: [&str; CM_N_RELATIONS] =
            ["registers", "memory", "merkle", "poseidon2", "range_check_8", "range_check_16", "range_check_20", "bitwise"];
        const P: u64 = (1 << 31) - 1;
        let mut out = Vec::new();
        for r in 0..CM_N_RELATIONS {
            let mut s = [0u64; 4];
            for k in 0..4 {
                s[k] = self.report.public_sum[r][k] as u64;
                for c in 0..CM_N_COMPONENTS {
                    s[k] += self.report.relation_sum[c][r][k] as u64;
                }
            }
            if s.iter().any(|w| w % P != 0) {
                out.push(NAMES[r]);
            }
        }
        out
    }
}

/// Twin of `debug_tools::assert_constraints` (crates/prover/src/debug_tools/assert_constraints.rs:24-60) on the GPU: the three
/// traces on their trace domains, relations drawn from a default channel, every constraint of every row tested and the LogUp
/// sums checked.  The reference panics on the first failure; this returns it.  `input` is consumed in place as by
/// `prove_cairo_m_hip`.  A library error (no GPU, out of memory) panics.
pub fn assert_constraints(input: &mut ProverInput) -> Result<(), ConstraintFailure> {
    ensure_init();
    let flat = Flat::new(input, MemoryOrder::AscendingAddress);
    let view = flat.view();
    let mut dev: *mut cm_device_input = std::ptr::null_mut();
    let rc = unsafe { cm_input_upload(&view, &mut dev) };
    assert!(rc == 0, "cm_input_upload: {}", last_error());
    let mut report: Box<cm_check_report> = Box::new(unsafe { std::mem::zeroed() });
    let rc = unsafe { cm_check_constraints(dev, std::ptr::null(), &mut *report) };
    unsafe { cm_input_free(dev) };
    assert!(rc == 0, "cm_check_constraints: {}", last_error());
    if report.status == 0 {
        return Ok(());
    }
    let message = unsafe { CStr::from_ptr(report.message.as_ptr()).to_string_lossy().into_owned() };
    Err(ConstraintFailure { report, message })
}

/// Why `assert_run_constraints` rejected a run: every segment's record (AIR report, link report, cell counts), the cells of every
/// link (`cap_per_link` slots per segment, `link_cells_written` of them filled) and the library's one-line summary of the first
/// bad link or segment.
#[derive(Clone)]
pub struct RunConstraintFailure {
    pub records: Vec<cm_run_check>,
    pub cells: Vec<cm_link_cell>,
    pub cap_per_link: usize,
    pub message: String,
}
impl std::fmt::Debug for RunConstraintFailure {
    fn fmt(&self, f: &mut std::fmt::Formatter<'_>) -> std::fmt::Result {
        write!(f, "RunConstraintFailure({})", self.message)
    }
}
impl RunConstraintFailure {
    /// the listed cells of the link between segment `i - 1` and segment `i`
    pub fn link_cells(&self, i: usize) -> &[cm_link_cell] {
        let n = self.records[i].link_cells_written as usize;
        &self.cells[i * self.cap_per_link..i * self.cap_per_link + n]
    }
}

/// `assert_constraints` for a whole run, before any proof is made (`cm_check_run`): every segment is adapted with the memory
/// carried on the device as under `prove_run_hip`, its AIR is checked, and its initial boundary memory is compared with its
/// predecessor's final one.  `Ok` means the run will prove and chain; the error names the segment, constraint and row, or the link
/// and the cells that make its roots differ (at most `cap_per_link` of them per link).  A library error (no GPU, a segment that
/// cannot be adapted) panics.
pub fn assert_run_constraints(
    initial_memory: &[u32],
    initial_heap: &[u32],
    ranges: [u32; 6],
    segments: &[RunSegment],
    cap_per_link: usize,
) -> Result<(), RunConstraintFailure> {
    ensure_init();
    let mut run: *mut cm_run = std::ptr::null_mut();
    let rc = unsafe {
        cm_run_begin(initial_memory.as_ptr(), (initial_memory.len() / 4) as u64, initial_heap.as_ptr(), (initial_heap.len() / 4) as u64, ranges.as_ptr(), &mut run)
    };
    assert!(rc == 0, "cm_run_begin: {}", last_error());
    let views: Vec<cm_run_segment> = segments
        .iter()
        .map(|s| cm_run_segment {
            trace: s.trace.as_ptr(),
            n_trace: (s.trace.len() / 2) as u64,
            memory_trace: s.memory_trace.as_ptr(),
            n_memory_trace: (s.memory_trace.len() / 5) as u64,
            n_memory_end: s.n_memory_end,
            n_heap_end: s.n_heap_end,
        })
        .collect();
    let ptrs: Vec<*const cm_run_segment> = views.iter().map(|v| v as *const cm_run_segment).collect();
    let mut records: Vec<cm_run_check> = vec![unsafe { std::mem::zeroed() }; segments.len()];
    let mut cells: Vec<cm_link_cell> = vec![cm_link_cell::default(); segments.len() * cap_per_link];
    let cells_ptr = if cap_per_link == 0 { std::ptr::null_mut() } else { cells.as_mut_ptr() };
    let rc = unsafe { cm_check_run(run, ptrs.as_ptr(), ptrs.len() as u32, std::ptr::null(), records.as_mut_ptr(), cells_ptr, cap_per_link as u64) };
    unsafe { cm_run_free(run) };
    assert!(rc == 0, "cm_check_run: status {rc}: {}", last_error());
    let bad = records.iter().enumerate().any(|(i, r)| {
        r.check.status != 0 || (i > 0 && (r.link.pc_equal == 0 || r.link.fp_equal == 0 || r.link.roots_equal == 0 || r.link_cells_total != 0))
    });
    if !bad {
        return Ok(());
    }
    Err(RunConstraintFailure { records, cells, cap_per_link, message: last_error() })
}

/// The openings of `addresses` under the initial (`which` = 0) or final (1) memory root of a device-resident input
/// (`cm_input_open_memory`), built on the GPU: the records and that root.  Every address is below 2^28; an absent cell opens as
/// the value zero.  A record is checked without the memory by `verify_memory_openings` (GPU, batched) or by
/// `ffi::cm_verify_memory_opening` (host code).
pub fn open_memory(input: *const cm_device_input, which: u32, addresses: &[u32]) -> Result<(Vec<CmMemOpening>, u32), String> {
    ensure_init();
    let mut out: Vec<CmMemOpening> = vec![unsafe { std::mem::zeroed() }; addresses.len()];
    let mut root: u32 = 0;
    let out_ptr = if addresses.is_empty() { std::ptr::null_mut() } else { out.as_mut_ptr() };
    let rc = unsafe { cm_input_open_memory(input, which, addresses.as_ptr(), addresses.len() as u64, out_ptr, &mut root) };
    if rc != 0 {
        return Err(last_error());
    }
    Ok((out, root))
}

/// Every opening checked against `root` on the GPU in one batch (`cm_verify_memory_openings`): one verdict per record; a malformed
/// record is a `false`, not an error.
pub fn verify_memory_openings(root: u32, openings: &[CmMemOpening]) -> Result<Vec<bool>, String> {
    ensure_init();
    let mut ok: Vec<u8> = vec![0; openings.len()];
    let rc = unsafe { cm_verify_memory_openings(root, openings.as_ptr(), openings.len() as u64, ok.as_mut_ptr(), 0) };
    if rc != 0 {
        return Err(last_error());
    }
    Ok(ok.iter().map(|v| *v != 0).collect())
}

/// The cells `start .. start + n_cells` under the initial (`which` = 0) or final (1) memory root of a device-resident input
/// (`cm_input_open_memory_range`), built on the GPU: the record, the values (four words per cell, an absent cell as zeros) and
/// that root.  At most 2^24 cells per call.  Checked without the memory by `verify_memory_range` (GPU) or by
/// `ffi::cm_verify_memory_range_host` (host code).
pub fn open_memory_range(input: *const cm_device_input, which: u32, start: u32, n_cells: u32) -> Result<(CmMemRangeOpening, Vec<u32>, u32), String> {
    ensure_init();
    let mut out: CmMemRangeOpening = unsafe { std::mem::zeroed() };
    let mut values: Vec<u32> = vec![0; 4 * (n_cells.min(1 << 24).max(1) as usize)];
    let mut root: u32 = 0;
    let rc = unsafe { cm_input_open_memory_range(input, which, start, n_cells, values.as_mut_ptr(), &mut out, &mut root) };
    if rc != 0 {
        return Err(last_error());
    }
    Ok((out, values, root))
}

/// A range checked against `root` on the GPU (`cm_verify_memory_range`): `values` holds four words per cell of the record; a
/// malformed record or value is a `false`, not an error.
pub fn verify_memory_range(root: u32, opening: &CmMemRangeOpening, values: &[u32]) -> Result<bool, String> {
    ensure_init();
    if opening.n_cells <= 1 << 24 && values.len() != 4 * opening.n_cells as usize {
        return Err(format!("{} value words for a range of {} cells", values.len(), opening.n_cells));
    }
    let mut ok: u8 = 0;
    let rc = unsafe { cm_verify_memory_range(root, opening, values.as_ptr(), &mut ok, 0) };
    if rc != 0 {
        return Err(last_error());
    }
    Ok(ok != 0)
}

/// A set of cells under one memory root (`cm_input_open_memory_set`): the strictly ascending addresses, four value words per
/// cell (an absent cell as zeros) and the sibling words, depth by depth from depth 28 up and by ascending node inside a depth: the
/// sibling of every node on a path of the set whose sibling is on none.
#[derive(Clone, Debug)]
pub struct MemSetOpening {
    pub addresses: Vec<u32>,
    pub values: Vec<u32>,
    pub siblings: Vec<u32>,
}

/// The cells `addresses` (any order, repeats allowed: sorted and made unique here) under the initial (`which` = 0) or final (1)
/// memory root of a device-resident input, built on the GPU: the record and that root.  At most 2^20 cells per call.  Checked
/// without the memory by `verify_memory_set` (GPU) or `memory_set_root` (host code).
pub fn open_memory_set(input: *const cm_device_input, which: u32, addresses: &[u32]) -> Result<(MemSetOpening, u32), String> {
    ensure_init();
    let mut a: Vec<u32> = addresses.to_vec();
    a.sort_unstable();
    a.dedup();
    let mut steps: [cm_mem_set_step; 29] = unsafe { std::mem::zeroed() };
    let (mut n_steps, mut need): (u32, u32) = (0, 0);
    let rc = unsafe { cm_mem_set_plan(a.as_ptr(), a.len() as u64, steps.as_mut_ptr(), 29, &mut n_steps, &mut need) };
    if rc != 0 {
        return Err(last_error());
    }
    let mut values: Vec<u32> = vec![0; 4 * a.len()];
    let mut siblings: Vec<u32> = vec![0; need as usize];
    let (mut got, mut root): (u32, u32) = (0, 0);
    let rc = unsafe {
        cm_input_open_memory_set(input, which, a.as_ptr(), a.len() as u64, values.as_mut_ptr(), siblings.as_mut_ptr(), need, &mut got, &mut root)
    };
    if rc != 0 {
        return Err(last_error());
    }
    siblings.truncate(got as usize);
    Ok((MemSetOpening { addresses: a, values, siblings }, root))
}

/// A set checked against `root` on the GPU (`cm_verify_memory_set`) -> (accepted, the root it folds to; 0 when malformed).  A
/// malformed record is a `false`, not an error.
pub fn verify_memory_set(root: u32, opening: &MemSetOpening) -> Result<(bool, u32), String> {
    ensure_init();
    if opening.values.len() != 4 * opening.addresses.len() {
        return Err(format!("{} value words for a set of {} cells", opening.values.len(), opening.addresses.len()));
    }
    let (mut ok, mut got): (u8, u32) = (0, 0);
    let rc = unsafe {
        cm_verify_memory_set(
            root,
            opening.addresses.as_ptr(),
            opening.addresses.len() as u64,
            opening.values.as_ptr(),
            opening.siblings.as_ptr(),
            opening.siblings.len() as u32,
            &mut ok,
            &mut got,
            0,
        )
    };
    if rc != 0 {
        return Err(last_error());
    }
    Ok((ok != 0, got))
}

/// The root a set folds to with its own values (`values` = None) or with others in their place (`cm_memory_set_root_host`): the
/// root AFTER a write that touched only cells of the set, from the sibling words opened BEFORE it.  Host code: touches no GPU.
pub fn memory_set_root(opening: &MemSetOpening, values: Option<&[u32]>) -> Result<u32, String> {
    let v: &[u32] = values.unwrap_or(&opening.values);
    if v.len() != 4 * opening.addresses.len() {
        return Err(format!("{} value words for a set of {} cells", v.len(), opening.addresses.len()));
    }
    let mut root: u32 = 0;
    let rc = unsafe {
        cm_memory_set_root_host(opening.addresses.as_ptr(), opening.addresses.len() as u64, v.as_ptr(), opening.siblings.as_ptr(), opening.siblings.len() as u32, &mut root)
    };
    if rc != 0 {
        return Err(last_error());
    }
    Ok(root)
}

/// A memory transition (`cm_input_open_transition`): strictly ascending addresses, their values under the root before and under
/// the root after, and ONE list of sibling words, a set opening's.  The old values fold to `root_before`, the new ones to
/// `root_after`: the two memories agree in every cell outside the set.
#[derive(Clone, Debug)]
pub struct MemTransition {
    pub addresses: Vec<u32>,
    pub old_values: Vec<u32>,
    pub new_values: Vec<u32>,
    pub siblings: Vec<u32>,
    pub root_before: u32,
    pub root_after: u32,
    pub n_zero_only: u32,
}

/// The cells a segment changes (`cm_input_write_set`), ascending: those whose value differs between the input's initial and final
/// boundary memory, and the count of cells present on one side only with an all-zero value, which are not listed.
pub fn write_set(input: *const cm_device_input) -> Result<(Vec<u32>, u64), String> {
    ensure_init();
    let (mut n, mut zero_only): (u64, u64) = (0, 0);
    let rc = unsafe { cm_input_write_set(input, std::ptr::null_mut(), 0, &mut n, &mut zero_only) };
    if rc != 0 {
        return Err(last_error());
    }
    let mut a: Vec<u32> = vec![0; n as usize];
    let rc = unsafe { cm_input_write_set(input, a.as_mut_ptr(), a.len() as u64, &mut n, &mut zero_only) };
    if rc != 0 {
        return Err(last_error());
    }
    a.truncate(n as usize);
    Ok((a, zero_only))
}

/// The transition of a device-resident input from its initial to its final memory root, built on the GPU: over the segment's
/// write set (`addresses` = None) or over the given cells (any order, repeats allowed), which must hold every cell that changes.
pub fn open_transition(input: *const cm_device_input, addresses: Option<&[u32]>) -> Result<MemTransition, String> {
    ensure_init();
    let mut h: *mut cm_mem_transition = std::ptr::null_mut();
    let rc = match addresses {
        None => unsafe { cm_input_open_transition(input, std::ptr::null(), 0, &mut h) },
        Some(list) => {
            let mut a: Vec<u32> = list.to_vec();
            a.sort_unstable();
            a.dedup();
            unsafe { cm_input_open_transition(input, a.as_ptr(), a.len() as u64, &mut h) }
        }
    };
    if rc != 0 {
        return Err(last_error());
    }
    take_transition(h)
}

/// The arrays of a `cm_mem_transition` handle, copied; the handle is freed.
fn take_transition(h: *mut cm_mem_transition) -> Result<MemTransition, String> {
    let mut v: cm_mem_transition_view = unsafe { std::mem::zeroed() };
    v.struct_size = std::mem::size_of::<cm_mem_transition_view>() as u32;
    let rc = unsafe { cm_mem_transition_get(h, &mut v) };
    let copy = |p: *const u32, k: usize| -> Vec<u32> {
        if k == 0 {
            Vec::new()
        } else {
            unsafe { std::slice::from_raw_parts(p, k) }.to_vec()
        }
    };
    let out = if rc == 0 {
        Ok(MemTransition {
            addresses: copy(v.addresses, v.n as usize),
            old_values: copy(v.old_values, 4 * v.n as usize),
            new_values: copy(v.new_values, 4 * v.n as usize),
            siblings: copy(v.siblings, v.n_siblings as usize),
            root_before: v.root_before,
            root_after: v.root_after,
            n_zero_only: v.n_zero_only,
        })
    } else {
        Err(last_error())
    };
    unsafe { cm_mem_transition_free(h) };
    out
}

/// A chain of transitions `parts[0] -> ... -> parts[k-1]` composed into ONE transition from the first root before to the last root
/// after over the union of their cells (`cm_compose_transitions`), from the records alone: `device` = false in host code (no GPU
/// needed), true on the GPU; the same bytes.  Nothing is hashed: the result is valid if every part is and the roots chain, so a
/// caller that does not trust its source verifies the result.  Input that is detectably broken (roots that do not chain, a seam
/// whose old value is not the previous new value, bad addresses or word counts) is an `Err` naming the cause.
pub fn compose_transitions(parts: &[MemTransition], device: bool) -> Result<MemTransition, String> {
    if device {
        ensure_init();
    }
    let views = transition_views(parts)?;
    let mut h: *mut cm_mem_transition = std::ptr::null_mut();
    let rc = unsafe { cm_compose_transitions(views.as_ptr(), views.len() as u32, if device { 1 } else { 0 }, &mut h) };
    if rc != 0 {
        return Err(last_error());
    }
    take_transition(h)
}

/// Transitions checked against their roots on the GPU in ONE batch (`cm_verify_memory_transitions`) -> per part what
/// `verify_memory_transition` gives for it alone: (accepted, the two roots it folds to; zeros when malformed).  The number of
/// launches does not depend on `parts.len()`; a malformed part is a `false` and does not disturb its neighbours.
pub fn verify_memory_transitions(parts: &[MemTransition]) -> Result<Vec<(bool, [u32; 2])>, String> {
    ensure_init();
    let views = transition_views(parts)?;
    let mut ok: Vec<u8> = vec![0; parts.len()];
    let mut got: Vec<u32> = vec![0; 2 * parts.len()];
    let rc = unsafe { cm_verify_memory_transitions(views.as_ptr(), views.len() as u32, ok.as_mut_ptr(), got.as_mut_ptr(), 0) };
    if rc != 0 {
        return Err(last_error());
    }
    Ok((0..parts.len()).map(|i| (ok[i] != 0, [got[2 * i], got[2 * i + 1]])).collect())
}

/// One filled `cm_mem_transition_view` per part, over the parts' own arrays
fn transition_views(parts: &[MemTransition]) -> Result<Vec<cm_mem_transition_view>, String> {
    let mut views: Vec<cm_mem_transition_view> = Vec::with_capacity(parts.len());
    for t in parts {
        if t.old_values.len() != 4 * t.addresses.len() || t.new_values.len() != 4 * t.addresses.len() {
            return Err(format!("{} old and {} new value words for a transition of {} cells", t.old_values.len(), t.new_values.len(), t.addresses.len()));
        }
        let mut v: cm_mem_transition_view = unsafe { std::mem::zeroed() };
        v.struct_size = std::mem::size_of::<cm_mem_transition_view>() as u32;
        v.root_before = t.root_before;
        v.root_after = t.root_after;
        v.n = t.addresses.len() as u32;
        v.n_siblings = t.siblings.len() as u32;
        v.n_zero_only = t.n_zero_only;
        v.addresses = t.addresses.as_ptr();
        v.old_values = t.old_values.as_ptr();
        v.new_values = t.new_values.as_ptr();
        v.siblings = t.siblings.as_ptr();
        views.push(v);
    }
    Ok(views)
}

/// A followed memory image (`cm_mem_image_*`): a copy of a run's memory with its partial Merkle tree, on the GPU (`device` = true)
/// or in host memory, independent of any prover handle.  It absorbs a segment's writes by re-hashing only the dirty paths, checks
/// itself against the proof's roots and opens cells under its current root.  A refused update is an `Err` and leaves the image
/// as it was.  The handle is freed when the value is dropped.
pub struct MemImage {
    handle: *mut cm_mem_image,
}

impl MemImage {
    /// The image of `addresses` (strictly ascending, below 2^28) with `values` (four words per cell, each below P).
    pub fn create(addresses: &[u32], values: &[u32], device: bool) -> Result<MemImage, String> {
        if device {
            ensure_init();
        }
        if values.len() != 4 * addresses.len() {
            return Err(format!("{} value words for an image of {} cells", values.len(), addresses.len()));
        }
        let mut h: *mut cm_mem_image = std::ptr::null_mut();
        let rc = unsafe { cm_mem_image_create(addresses.as_ptr(), values.as_ptr(), addresses.len() as u64, if device { 1 } else { 0 }, &mut h) };
        if rc != 0 {
            return Err(last_error());
        }
        Ok(MemImage { handle: h })
    }

    /// The image's current root.
    pub fn root(&self) -> Result<u32, String> {
        let mut root: u32 = 0;
        let rc = unsafe { cm_mem_image_root(self.handle, &mut root) };
        if rc != 0 {
            return Err(last_error());
        }
        Ok(root)
    }

    /// `t`'s new values written to its addresses, from `t.root_before` to `t.root_after`, both checked, as are the old values
    /// (`cm_mem_image_apply_transition`).  The sibling words are never read: a bare transition (addresses, both value planes, two
    /// roots) is enough.  Returns the new root.
    pub fn apply_transition(&mut self, t: &MemTransition) -> Result<u32, String> {
        if t.old_values.len() != 4 * t.addresses.len() || t.new_values.len() != 4 * t.addresses.len() {
            return Err(format!("{} old and {} new value words for a transition of {} cells", t.old_values.len(), t.new_values.len(), t.addresses.len()));
        }
        let mut v: cm_mem_transition_view = unsafe { std::mem::zeroed() };
        v.struct_size = std::mem::size_of::<cm_mem_transition_view>() as u32;
        v.root_before = t.root_before;
        v.root_after = t.root_after;
        v.n = t.addresses.len() as u32;
        v.n_zero_only = t.n_zero_only;
        v.addresses = t.addresses.as_ptr();
        v.old_values = t.old_values.as_ptr();
        v.new_values = t.new_values.as_ptr();
        let rc = unsafe { cm_mem_image_apply_transition(self.handle, &v, std::ptr::null_mut()) };
        if rc != 0 {
            return Err(last_error());
        }
        self.root()
    }

    /// One transition each to DIFFERENT device images in one call, through one ladder of launches (`cm_mem_images_apply`): per
    /// part `Ok(the new root)`, or `Err((status, message))` in the words `apply_transition` would use, the image as it was; a
    /// refused part does not disturb the others.  The outer `Err` is a call refused as a whole (one image twice, no parts, more
    /// than 2^20 cells in all) or a missing device.
    pub fn apply_many(updates: &mut [(&mut MemImage, &MemTransition)]) -> Result<Vec<Result<u32, (i32, String)>>, String> {
        ensure_init();
        let mut parts: Vec<cm_mem_image_update> = Vec::with_capacity(updates.len());
        for (image, t) in updates.iter() {
            if t.old_values.len() != 4 * t.addresses.len() || t.new_values.len() != 4 * t.addresses.len() {
                return Err(format!("{} old and {} new value words for a transition of {} cells", t.old_values.len(), t.new_values.len(), t.addresses.len()));
            }
            let mut p: cm_mem_image_update = unsafe { std::mem::zeroed() };
            p.struct_size = std::mem::size_of::<cm_mem_image_update>() as u32;
            p.n = t.addresses.len() as u32;
            p.img = image.handle;
            p.addresses = t.addresses.as_ptr();
            p.new_values = t.new_values.as_ptr();
            p.old_values = t.old_values.as_ptr();
            p.root_before = &t.root_before;
            p.root_after = &t.root_after;
            parts.push(p);
        }
        let blank = cm_mem_image_result { status: -1, root: 0, message: [0u8; 248] };
        let mut results: Vec<cm_mem_image_result> = vec![blank; parts.len()];
        let rc = unsafe { cm_mem_images_apply(parts.as_ptr(), parts.len() as u32, results.as_mut_ptr()) };
        // a call refused as a whole writes no result; a call that judged every part returns the lowest bad part's status
        if rc != 0 && (results.is_empty() || results.iter().any(|r| r.status == -1) || results.iter().all(|r| r.status != rc)) {
            return Err(last_error());
        }
        Ok(results
            .iter()
            .map(|r| {
                if r.status == 0 {
                    return Ok(r.root);
                }
                let end = r.message.iter().position(|&b| b == 0).unwrap_or(r.message.len());
                Err((r.status, String::from_utf8_lossy(&r.message[..end]).into_owned()))
            })
            .collect())
    }

    /// One set each under device images in one call, through one chain of launches and one round trip
    /// (`cm_mem_images_open_memory_sets`); several parts may name one image.  Addresses in any order, repeats allowed: sorted and
    /// made unique here, per part.  Per part `Ok((the record, the root it opens under))`, or `Err((status, message))` in the words
    /// `open_set` would use; a bad part does not disturb the others.  The outer `Err` is a call refused as a whole (no parts, more
    /// than 2^20 cells in all) or a missing device.
    pub fn open_sets_many(requests: &[(&MemImage, &[u32])]) -> Result<Vec<Result<(MemSetOpening, u32), (i32, String)>>, String> {
        ensure_init();
        let mut sets: Vec<(Vec<u32>, Vec<u32>, Vec<u32>)> = Vec::with_capacity(requests.len());
        for (_, addresses) in requests.iter() {
            let mut a: Vec<u32> = addresses.to_vec();
            a.sort_unstable();
            a.dedup();
            let mut steps: [cm_mem_set_step; 29] = unsafe { std::mem::zeroed() };
            let (mut n_steps, mut need): (u32, u32) = (0, 0);
            let rc = unsafe { cm_mem_set_plan(a.as_ptr(), a.len() as u64, steps.as_mut_ptr(), 29, &mut n_steps, &mut need) };
            if rc != 0 {
                return Err(last_error());
            }
            let values: Vec<u32> = vec![0; 4 * a.len()];
            let siblings: Vec<u32> = vec![0; need as usize];
            sets.push((a, values, siblings));
        }
        let mut parts: Vec<cm_mem_set_request> = Vec::with_capacity(requests.len());
        for ((image, _), (a, values, siblings)) in requests.iter().zip(sets.iter_mut()) {
            let mut p: cm_mem_set_request = unsafe { std::mem::zeroed() };
            p.struct_size = std::mem::size_of::<cm_mem_set_request>() as u32;
            p.n = a.len() as u32;
            p.img = image.handle;
            p.addresses = a.as_ptr();
            p.values = values.as_mut_ptr();
            p.siblings = siblings.as_mut_ptr();
            p.cap_siblings = siblings.len() as u32;
            parts.push(p);
        }
        let blank = cm_mem_set_result { status: -1, root: 0, n_siblings: 0, reserved: 0, message: [0u8; 240] };
        let mut results: Vec<cm_mem_set_result> = vec![blank; parts.len()];
        let rc = unsafe { cm_mem_images_open_memory_sets(parts.as_ptr(), parts.len() as u32, results.as_mut_ptr()) };
        // a call refused as a whole writes no result; a call that judged every part returns the lowest bad part's status
        if rc != 0 && (results.is_empty() || results.iter().any(|r| r.status == -1) || results.iter().all(|r| r.status != rc)) {
            return Err(last_error());
        }
        Ok(results
            .iter()
            .zip(sets.into_iter())
            .map(|(r, (a, values, mut siblings))| {
                if r.status == 0 {
                    siblings.truncate(r.n_siblings as usize);
                    return Ok((MemSetOpening { addresses: a, values, siblings }, r.root));
                }
                let end = r.message.iter().position(|&b| b == 0).unwrap_or(r.message.len());
                Err((r.status, String::from_utf8_lossy(&r.message[..end]).into_owned()))
            })
            .collect())
    }

    /// The cells `addresses` (any order, repeats allowed: sorted and made unique here) under the image's current root, built on
    /// the GPU (`cm_mem_image_open_memory_set`; device images only): the record and that root.
    pub fn open_set(&self, addresses: &[u32]) -> Result<(MemSetOpening, u32), String> {
        let mut a: Vec<u32> = addresses.to_vec();
        a.sort_unstable();
        a.dedup();
        let mut steps: [cm_mem_set_step; 29] = unsafe { std::mem::zeroed() };
        let (mut n_steps, mut need): (u32, u32) = (0, 0);
        let rc = unsafe { cm_mem_set_plan(a.as_ptr(), a.len() as u64, steps.as_mut_ptr(), 29, &mut n_steps, &mut need) };
        if rc != 0 {
            return Err(last_error());
        }
        let mut values: Vec<u32> = vec![0; 4 * a.len()];
        let mut siblings: Vec<u32> = vec![0; need as usize];
        let (mut got, mut root): (u32, u32) = (0, 0);
        let rc = unsafe {
            cm_mem_image_open_memory_set(self.handle, a.as_ptr(), a.len() as u64, values.as_mut_ptr(), siblings.as_mut_ptr(), need, &mut got, &mut root)
        };
        if rc != 0 {
            return Err(last_error());
        }
        siblings.truncate(got as usize);
        Ok((MemSetOpening { addresses: a, values, siblings }, root))
    }
}

impl Drop for MemImage {
    fn drop(&mut self) {
        unsafe { cm_mem_image_free(self.handle) };
    }
}

/// A transition checked against its two roots on the GPU in one fold (`cm_verify_memory_transition`) -> (accepted, the two roots
/// it folds to; zeros when malformed).  A malformed record is a `false`, not an error.
pub fn verify_memory_transition(t: &MemTransition) -> Result<(bool, [u32; 2]), String> {
    ensure_init();
    if t.old_values.len() != 4 * t.addresses.len() || t.new_values.len() != 4 * t.addresses.len() {
        return Err(format!("{} old and {} new value words for a transition of {} cells", t.old_values.len(), t.new_values.len(), t.addresses.len()));
    }
    let mut ok: u8 = 0;
    let mut got = [0u32; 2];
    let rc = unsafe {
        cm_verify_memory_transition(
            t.root_before,
            t.root_after,
            t.addresses.as_ptr(),
            t.addresses.len() as u64,
            t.old_values.as_ptr(),
            t.new_values.as_ptr(),
            t.siblings.as_ptr(),
            t.siblings.len() as u32,
            &mut ok,
            got.as_mut_ptr(),
            0,
        )
    };
    if rc != 0 {
        return Err(last_error());
    }
    Ok((ok != 0, got))
}

/// The passes of a 2^`log_n` transform as the library runs it (`cm_fft_plan`), in layer order: `[lo, hi, tile_log, M]` per pass,
/// `tile_log` 0 = the generic kernel.  Host code: touches no GPU.
pub fn fft_plan(log_n: u32) -> Result<Vec<[u32; 4]>, String> {
    let mut out = [[0u32; 4]; 8];
    let mut n: u32 = 0;
    let rc = unsafe { cm_fft_plan(log_n, out.as_mut_ptr(), &mut n) };
    if rc != 0 {
        return Err(last_error());
    }
    Ok(out[..n as usize].to_vec())
}

/// Whether `cm_interpolate_extend` takes the fused sweep at 2^`log_n` rows under the current tuning (`cm_fft_extend_fused`).
pub fn fft_extend_fused(log_n: u32) -> Result<bool, String> {
    let mut fused: u32 = 0;
    let rc = unsafe { cm_fft_extend_fused(log_n, &mut fused) };
    if rc != 0 {
        return Err(last_error());
    }
    Ok(fused != 0)
}

/// The launches of a Merkle commitment of columns with these log sizes (`cm_merkle_plan`), in launch order: per launch
/// `[kind, hi, lo, has_prev, PREV, NC, npw, wide_mask, first_column, columns of layer hi, hi - 1, ..]` (include/cairom_hip.h).
/// Host code: touches no GPU.
pub fn merkle_plan(col_logs: &[u32]) -> Result<Vec<[u32; CM_MERKLE_PLAN_WORDS]>, String> {
    let mut out = [[0u32; CM_MERKLE_PLAN_WORDS]; 33];
    let mut n: u32 = 0;
    let rc = unsafe { cm_merkle_plan(col_logs.as_ptr(), col_logs.len() as u32, out.as_mut_ptr(), 33, &mut n) };
    if rc != 0 {
        return Err(last_error());
    }
    Ok(out[..n as usize].to_vec())
}

/// What `cm_merkle_commit_layer` launches for such a layer (`cm_merkle_layer_npw`): 0 = `k_merkle_layer`, else the chunks per
/// wave of `k_merkle_narrow`.  Host code: touches no GPU.
pub fn merkle_layer_npw(log_size: u32, has_prev: bool, n_cols: u32) -> Result<u32, String> {
    let mut npw: u32 = 0;
    let rc = unsafe { cm_merkle_layer_npw(log_size, has_prev as u32, n_cols, &mut npw) };
    if rc != 0 {
        return Err(last_error());
    }
    Ok(npw)
}

/// The host adapter over a caller-supplied runner segment (`cm_adapt_segment_host`): the `cm_host_input` that `cm_vm_run`
/// returns, built without a GPU; the log defines every step's opcode.  The caller frees it with `cm_host_input_free`.
pub fn adapt_segment_host(seg: &cm_runner_segment) -> Result<*mut cm_host_input, String> {
    let mut out: *mut cm_host_input = std::ptr::null_mut();
    let rc = unsafe { cm_adapt_segment_host(seg, &mut out) };
    if rc != 0 {
        return Err(last_error());
    }
    Ok(out)
}

/// The public entries a device input holds (`cm_device_input_public_entries`; `which`: 0 program, 1 input, 2 output): per
/// address of the range `[present, address, value[4], clock]`, as its proof will carry them.  Host memory: touches no GPU.
pub fn device_input_public_entries(input: *const cm_device_input, which: u32) -> Result<Vec<[u32; 7]>, String> {
    let mut n: u64 = 0;
    let rc = unsafe { cm_device_input_public_entries(input, which, std::ptr::null_mut(), 0, &mut n) };
    if rc != 0 {
        return Err(last_error());
    }
    let mut out = vec![[0u32; 7]; n as usize];
    let rc = unsafe { cm_device_input_public_entries(input, which, out.as_mut_ptr() as *mut u32, n, &mut n) };
    if rc != 0 {
        return Err(last_error());
    }
    Ok(out)
}

/// `cm_merkle_commit_layers`: the root of the mixed-degree tree over `cols` and every stored layer, largest first, 8 words per node.
pub fn merkle_commit_layers(cols: &[cm_handle], col_logs: &[u32]) -> Result<([u8; 32], Vec<u32>), String> {
    ensure_init();
    assert_eq!(cols.len(), col_logs.len());
    let max_log = col_logs.iter().copied().max().unwrap_or(0);
    let mut layers = vec![0u32; ((2usize << max_log) - 1) * 8];
    let mut root = [0u8; 32];
    let rc = unsafe {
        cm_merkle_commit_layers(cols.as_ptr(), col_logs.as_ptr(), cols.len() as u32, root.as_mut_ptr(), layers.as_mut_ptr(), layers.len() as u64, 0)
    };
    if rc != 0 {
        return Err(last_error());
    }
    Ok((root, layers))
}

/// Twin of `debug_tools::relation_tracker::track_and_summarize_relations` (relation_tracker.rs:21-31, the `.cleaned()` summary) on
/// the GPU: relation name -> the tuples (values without trailing zeros) whose multiplicities do not sum to zero, with their net
/// multiplicity.  Only the relations whose sums do not cancel are tracked, so a valid input returns an empty map at the cost of
/// `assert_constraints`.  The public data takes part with the terms of `PublicData::initial_logup_sum`.  `input` is consumed in
/// place as by `prove_cairo_m_hip`.  A library error (no GPU, out of memory) panics.
pub fn track_and_summarize_relations(input: &mut ProverInput) -> std::collections::BTreeMap<&'static str, Vec<(Vec<stwo_prover::core::fields::m31::M31>, stwo_prover::core::fields::m31::M31)>> {
    use stwo_prover::core::fields::m31::M31;
    const NAMES: [&str; CM_N_RELATIONS] =
        ["registers", "memory", "merkle", "poseidon2", "range_check_8", "range_check_16", "range_check_20", "bitwise"];
    ensure_init();
    let flat = Flat::new(input, MemoryOrder::AscendingAddress);
    let view = flat.view();
    let mut dev: *mut cm_device_input = std::ptr::null_mut();
    let rc = unsafe { cm_input_upload(&view, &mut dev) };
    assert!(rc == 0, "cm_input_upload: {}", last_error());
    let mut cap: u64 = 4096;
    let mut entries: Vec<cm_relation_entry> = Vec::new();
    loop {
        entries.resize(cap as usize, unsafe { std::mem::zeroed() });
        let mut n_total: u64 = 0;
        let rc = unsafe { cm_track_relations(dev, std::ptr::null(), 0, std::ptr::null_mut(), entries.as_mut_ptr(), cap, &mut n_total) };
        if rc != 0 {
            unsafe { cm_input_free(dev) };
            panic!("cm_track_relations: {}", last_error());
        }
        if n_total <= cap {
            entries.truncate(n_total as usize);
            break;
        }
        cap = n_total;
    }
    unsafe { cm_input_free(dev) };
    let mut out: std::collections::BTreeMap<&'static str, Vec<(Vec<M31>, M31)>> = std::collections::BTreeMap::new();
    for e in entries.iter() {
        let values: Vec<M31> = e.values[..e.n_values as usize].iter().map(|v| M31::from_u32_unchecked(*v)).collect();
        out.entry(NAMES[e.relation as usize]).or_default().push((values, M31::from_u32_unchecked(e.multiplicity)));
    }
    out
}

/// Device memory a proof of `input` needs under `config` (`None` = REGULAR_96_BITS), computed on the host without a GPU:
/// `(input_bytes, working_bytes, cached_bytes)`.  `working_bytes` is an upper bound of what one proof adds to its thread's device
/// pool; a host that keeps several proofs in flight sizes `set_memory_budget` from it.  `world` = 1 for `prove_cairo_m_hip`,
/// 2 / 4 / 8 for one rank of a sharded proof.
pub fn estimate_memory(input: &mut ProverInput, config: Option<cm_pcs_config>, world: u32) -> Result<(u64, u64, u64), String> {
    let flat = Flat::new(input, MemoryOrder::AscendingAddress);
    let view = flat.view();
    let mut e: cm_mem_estimate = unsafe { std::mem::zeroed() };
    e.struct_size = std::mem::size_of::<cm_mem_estimate>() as u32;
    let cfg_ptr = match config.as_ref() {
        Some(c) => c as *const cm_pcs_config,
        None => std::ptr::null(),
    };
    let rc = unsafe { cm_estimate_memory(&view, cfg_ptr, world, &mut e) };
    if rc != 0 {
        return Err(last_error());
    }
    Ok((e.input_bytes, e.working_bytes, e.cached_bytes))
}

/// Bytes the proof pipelines (`cm_prove_many*`) may keep live in device memory, process-wide; 0 = no budget.
pub fn set_memory_budget(bytes: u64) {
    let rc = unsafe { cm_set_memory_budget(bytes) };
    assert!(rc == 0, "cm_set_memory_budget: {}", last_error());
}

/// The process-wide device-memory counters (live / reserved bytes, their peaks, driver allocations, proofs in flight).
pub fn memory_stats() -> cm_mem_stats {
    let mut s: cm_mem_stats = unsafe { std::mem::zeroed() };
    s.struct_size = std::mem::size_of::<cm_mem_stats>() as u32;
    let rc = unsafe { cm_mem_stats_get(&mut s) };
    assert!(rc == 0, "cm_mem_stats_get: {}", last_error());
    s
}

// spl_nest_host.h -- the host half of spl_nest_reserve_device / spl_nest_index_device / spl_nest_step_device (spl_k_nest.h): the refusals
// (all of them before the device is touched), the index's four launches and the step's one.  The table and the index are the caller's
// device memory; the tables of the vocabulary are spl_dfa_host.h's.  The INDEX BUILD may allocate (Ctx::d_nsscr, grow-only: the touching
// bitmap, one word per word of the rows, and the per-state counts) and synchronises the stream ONCE, to read the number of dependent
// entries: it is refused when they do not fit dep_cap.  The count-scan-write driver of spl_seqscan_host.h does not fit: it scans uint64
// counts per sequence over block sums into a CSR of uint64 offsets, here at most 4096 uint32 counts go into dep_off in one workgroup.  The
// STEP neither allocates nor synchronises after spl_nest_reserve_device.
#pragma once
namespace {

static_assert(NS_MAX_DEPTH == SPL_NEST_MAX_DEPTH && NS_STATE_WORDS == SPL_NEST_STATE_WORDS && NS_MAX_RET == SPL_NEST_MAX_RET,
              "spl_k_nest.h and splintr_hip.h must agree on the layout");
static_assert(SPL_NEST_KEEP_FREE == SPL_DFA_KEEP_FREE && SPL_NEST_I64 == SPL_DFA_I64 && SPL_NEST_MAX_END == SPL_DFA_MAX_END, "the nest calls take the regex guide's flags");
static_assert(SPL_NEST_TABLE_BYTES(3, 2) == 3 * 769 + 2 * 32 && SPL_NEST_INDEX_BYTES(3, 5, 7) == 3 * 8 * 4 + 4 * 4 + 7 * 4 + 3, "the macros size a table and an index");
static_assert(sizeof(((spl_nest_opts*)nullptr)->end_ids) == sizeof(((DfIn*)nullptr)->end_ids), "the END ids travel by value");

int nest_reserve_device(spl_tokenizer* t) {
    if (!t) return fail(SPL_EINVAL, "spl_nest_reserve_device: null handle");
    Ctx* c = t->ctx[0].get();
    HIP_TRY(hipSetDevice(c->device));
    return upload_heal(t, c);
}

// what every call asks of a table and a row width, beyond what the regex guide asks
int nest_refuse_shape(const spl_tokenizer* t, const std::string& who, const uint8_t* d_table, uint32_t n_states, uint32_t n_ret, uint32_t n_words) {
    SPL_TRY(dfa_refuse_shape(t, who, d_table, n_states, n_words));
    if (n_ret > SPL_NEST_MAX_RET) return fail(SPL_EINVAL, who + ": n_ret is " + std::to_string(n_ret) + ", above SPL_NEST_MAX_RET (4096)");
    return SPL_OK;
}

// the parts of an index
struct NsIndexAt {
    uint32_t* rows; uint32_t* dep_off; uint32_t* dep_ids; uint8_t* some; uint32_t stride;
    NsIndexAt(void* d_index, uint32_t n_states, uint32_t n_words, uint32_t dep_cap) {
        stride = df_stride(n_words);
        rows = reinterpret_cast<uint32_t*>(d_index);
        dep_off = rows + (size_t)n_states * stride;
        dep_ids = dep_off + n_states + 1;
        some = reinterpret_cast<uint8_t*>(dep_ids + dep_cap);
    }
};

int nest_index_device(spl_tokenizer* t, const uint8_t* d_table, uint32_t n_states, uint32_t n_ret, uint32_t n_words, int32_t* d_index, uint32_t dep_cap,
                      uint32_t* n_dep, hipStream_t st) {
    const std::string who = "spl_nest_index_device";
    if (!t) return fail(SPL_EINVAL, who + ": null handle");
    SPL_TRY(nest_refuse_shape(t, who, d_table, n_states, n_ret, n_words));
    if (!d_index) return fail(SPL_EINVAL, who + ": d_index is null");
    if (col_misaligned(d_index, 4)) return fail(SPL_EINVAL, who + ": d_index is not 4-byte aligned");
    if ((const void*)d_index == (const void*)d_table) return fail(SPL_EINVAL, who + ": d_index coincides with d_table");
    if (!n_dep) return fail(SPL_EINVAL, who + ": n_dep is null");

    Ctx* c = t->ctx[0].get();
    HIP_TRY(hipSetDevice(c->device));
    SPL_TRY(upload_heal(t, c));
    const NsIndexAt ix(d_index, n_states, n_words, dep_cap);
    const uint32_t stride = ix.stride;
    const uint64_t need = (uint64_t)n_states * stride + n_states;
    SPL_TRY(c->d_nsscr.grow(&c->nsscr_cap, need, need));
    uint32_t* touch = c->d_nsscr.get();
    uint32_t* cnt = touch + (size_t)n_states * stride;
    const NsTab d = ns_tab(d_table, n_states, n_ret);
    const uint32_t per = DF_INDEX_NT / DF_WAVE, waves = stride / 2;                 // (a wavefront owns 64 ids: two words of every row)
    hipLaunchKernelGGL(k_nest_index, dim3((waves + per - 1) / per, (n_states + DF_INDEX_STATES - 1) / DF_INDEX_STATES), dim3(DF_INDEX_NT), 0, st,
                       dfa_hl_tab(c), d, stride, ix.rows, touch);
    HIP_TRY(hipGetLastError());
    const uint32_t grid = (n_states + NS_NT / DF_WAVE - 1) / (NS_NT / DF_WAVE);
    hipLaunchKernelGGL(k_nest_count, dim3(grid), dim3(NS_NT), 0, st, (const uint32_t*)ix.rows, (const uint32_t*)touch, stride, n_states, ix.some, cnt);
    hipLaunchKernelGGL(k_nest_scan, dim3(1), dim3(NS_SCAN_NT), 0, st, (const uint32_t*)cnt, n_states, ix.dep_off);
    HIP_TRY(hipGetLastError());
    // the ONE synchronisation: do the dependent entries fit
    uint32_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, ix.dep_off + n_states, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *n_dep = total;
    if (total > dep_cap)
        return fail(SPL_ECAPACITY, who + ": dep_cap is too small: " + std::to_string(dep_cap) + " entries for " + std::to_string(total) + " dependent ids");
    if (total) {
        hipLaunchKernelGGL(k_nest_write, dim3(grid), dim3(NS_NT), 0, st, (const uint32_t*)touch, stride, n_states, (const uint32_t*)ix.dep_off, ix.dep_ids, dep_cap);
        HIP_TRY(hipGetLastError());
    }
    return SPL_OK;
}

int nest_refuse_step(const spl_tokenizer* t, const std::string& who, const spl_nest_in* in, const spl_nest_opts* o, const spl_nest_out* out) {
    if (!t) return fail(SPL_EINVAL, who + ": null handle");
    if (!in) return fail(SPL_EINVAL, who + ": the input struct is null");
    if (!o) return fail(SPL_EINVAL, who + ": the options are null");
    if (!out) return fail(SPL_EINVAL, who + ": the output struct is null");
    SPL_TRY(refuse_struct_size(who, "spl_nest_in", in->struct_size, sizeof(spl_nest_in), "the struct"));
    SPL_TRY(refuse_struct_size(who, "spl_nest_opts", o->struct_size, sizeof(spl_nest_opts), "the struct"));
    SPL_TRY(refuse_struct_size(who, "spl_nest_out", out->struct_size, sizeof(spl_nest_out), "the struct"));
    SPL_TRY(refuse_unknown_bits(who, "flag", o->flags, SPL_NEST_KEEP_FREE | SPL_NEST_I64));
    if (in->n_seqs >= (1ull << 31)) return fail(SPL_EINVAL, who + ": n_seqs >= 2^31");
    SPL_TRY(nest_refuse_shape(t, who, in->d_table, in->n_states, in->n_ret, o->n_words));
    if (!o->max_depth || o->max_depth > SPL_NEST_MAX_DEPTH)
        return fail(SPL_EINVAL, who + ": max_depth is " + std::to_string(o->max_depth) + ", not in 1 .. SPL_NEST_MAX_DEPTH (64)");
    if (!in->d_index) return fail(SPL_EINVAL, who + ": d_index is null");
    if (in->index_bytes < SPL_NEST_INDEX_BYTES(in->n_states, o->n_words, in->dep_cap))
        return fail(SPL_EINVAL, who + ": index_bytes is " + std::to_string(in->index_bytes) + ": the index is too small for dep_cap " + std::to_string(in->dep_cap));
    if (!in->d_state_in) return fail(SPL_EINVAL, who + ": d_state_in is null");
    if (!out->d_state_out) return fail(SPL_EINVAL, who + ": d_state_out is null");
    if (!out->d_mask) return fail(SPL_EINVAL, who + ": d_mask is null");
    if (!in->d_ids && in->n_seqs && in->row_len) return fail(SPL_EINVAL, who + ": d_ids is null");
    if (col_misaligned(in->d_ids, (o->flags & SPL_NEST_I64) ? 8 : 4)) return fail(SPL_EINVAL, who + ": d_ids is not aligned to its element type (int32, or int64 with SPL_NEST_I64)");
    if (col_misaligned(in->d_len, 4) || col_misaligned(out->d_mask, 4) || col_misaligned(in->d_index, 4))
        return fail(SPL_EINVAL, who + ": d_len, d_index or d_mask is not 4-byte aligned");
    if (col_misaligned(in->d_state_in, 8) || col_misaligned(out->d_state_out, 8)) return fail(SPL_EINVAL, who + ": a state array is not 8-byte aligned");
    // outputs may coincide with nothing but themselves: state out with state in is the one exception
    const void* ins[] = {in->d_ids, in->d_len, in->d_state_in, in->d_table, in->d_index};
    const void* outs[] = {out->d_state_out, out->d_mask, out->d_live};
    const char* on[] = {"d_state_out", "d_mask", "d_live"};
    for (int i = 0; i < 3; i++) {
        if (!outs[i]) continue;
        for (int j = 0; j < 5; j++)
            if (outs[i] == ins[j] && !(i == 0 && j == 2)) return fail(SPL_EINVAL, who + ": " + on[i] + " coincides with an input array");
        for (int j = 0; j < i; j++)
            if (outs[i] == outs[j]) return fail(SPL_EINVAL, who + ": " + on[i] + " coincides with " + on[j]);
    }
    if (!o->n_end) return fail(SPL_EINVAL, who + ": n_end is 0: no sequence could ever finish");
    if (o->n_end > SPL_NEST_MAX_END) return fail(SPL_EINVAL, who + ": n_end is above SPL_NEST_MAX_END (8)");
    for (uint32_t i = 0; i < o->n_end; i++)
        if ((uint64_t)o->end_ids[i] >= (uint64_t)o->n_words * 32)
            return fail(SPL_EINVAL, who + ": END id " + std::to_string(o->end_ids[i]) + " is at or above 32 * n_words");
    return SPL_OK;
}

int nest_step_device(spl_tokenizer* t, const spl_nest_in* in, const spl_nest_opts* o, const spl_nest_out* out, hipStream_t st) {
    SPL_TRY(nest_refuse_step(t, "spl_nest_step_device", in, o, out));
    Ctx* c = t->ctx[0].get();
    HIP_TRY(hipSetDevice(c->device));
    SPL_TRY(upload_heal(t, c));
    const uint64_t B = in->n_seqs;
    if (!B) return SPL_OK;
    const NsIndexAt ix(const_cast<int32_t*>(in->d_index), in->n_states, o->n_words, in->dep_cap);
    const NsIndex x{ix.rows, ix.dep_off, ix.dep_ids, ix.some, ix.stride, in->dep_cap};
    DfIn a{};
    a.ids = in->d_ids; a.len = in->d_len; a.state_in = in->d_state_in; a.n_seqs = B;
    a.row_len = in->row_len; a.flags = o->flags; a.n_words = o->n_words;
    a.v4 = o->n_words % 4 == 0 && !col_misaligned(out->d_mask, 16) && !col_misaligned(in->d_index, 16) ? 1u : 0u;
    a.n_end = o->n_end;
    for (uint32_t i = 0; i < o->n_end; i++) a.end_ids[i] = o->end_ids[i];
    const NsOut co{out->d_state_out, reinterpret_cast<uint32_t*>(out->d_mask), out->d_live, o->n_words};
    const uint32_t gy = (uint32_t)std::min<uint64_t>(B, 65535), gz = (uint32_t)((B + gy - 1) / gy);
    hipLaunchKernelGGL(k_nest_step, dim3(1, gy, gz), dim3(DF_WAVE), 0, st, a, dfa_hl_tab(c), ns_tab(in->d_table, in->n_states, in->n_ret), x, NsStep{o->max_depth}, co);
    HIP_TRY(hipGetLastError());
    return SPL_OK;
}

}  // namespace

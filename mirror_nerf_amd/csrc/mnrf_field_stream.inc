// mnrf_field_stream.inc -- global -> LDS weight stream shared by the field kernel tunings.
// The includer defines CHUNK_BYTES (LDS staging granule), RING_SLOTS, PIECES (1-KiB LDS-DMA
// pieces each wave issues per chunk), and `smem`.
// ------------------------------------------------------------------ weight stream
// The packed image is consumed strictly in order, chunk by chunk, through a ring of
// three LDS slots: one being read, one landed, one in flight.  `advance` is called PF tiles
// before the first read of a chunk, so A operands can be prefetched across chunk seams.
struct Stream {
    const char* src;   // this lane's source of chunk 0 (wave and lane offsets included)
    int next;          // next chunk to issue
    int end;           // chunks in this stream
    int rd_slot;       // ring slot of the newest readable chunk
};


__device__ __forceinline__ void issue_chunk(const Stream& st, int chunk, int wave) {
    const char* g = st.src + (long long)chunk * CHUNK_BYTES;
    char* l = smem + (chunk % RING_SLOTS) * CHUNK_BYTES + wave * PIECES * TILE_BYTES;
    // PIECES 1-KiB pieces per wave: lane i's 16 bytes land at l + 16*i (wave-uniform base)
#pragma unroll
    for (int i = 0; i < PIECES; ++i)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(g + i * TILE_BYTES),
                                         (__attribute__((address_space(3))) void*)(l + i * TILE_BYTES), 16, 0, 0);
}

// Make chunk (st.next-1) readable and start the copy of chunk st.next.  The slot that copy
// overwrites held chunk st.next-3, which every wave finished before reaching this barrier.
__device__ __forceinline__ void advance(Stream& st, int wave) {
    // My pieces of chunk next-1 have landed (vmcnt); everybody's have (barrier).  A raw s_barrier,
    // not __syncthreads(): LDS reads of the current chunk may stay in flight across it (they target
    // a slot that is not rewritten before the next advance), so lgkmcnt is deliberately not drained.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    st.rd_slot = st.rd_slot == RING_SLOTS - 1 ? 0 : st.rd_slot + 1;   // slot of chunk next-1
    if (st.next < st.end) issue_chunk(st, st.next, wave);
    st.next += 1;
}

__device__ __forceinline__ void open_stream(Stream& st, const float* base, int n_tiles, int wave, int lane) {
    __syncthreads();   // all waves are done with the ring (previous stream)
    st.src = (const char*)base + wave * PIECES * TILE_BYTES + lane * 16;
    st.end = n_tiles * TILE_BYTES / CHUNK_BYTES;   // n_tiles counts 1-KiB units
    st.next = 1;
    st.rd_slot = RING_SLOTS - 1;   // the first advance() makes slot 0 (chunk 0) the readable one
    issue_chunk(st, 0, wave);
}

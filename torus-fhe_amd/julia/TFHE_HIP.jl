# TFHE_HIP.jl -- thin Julia host layer over libthfhe_hip.so (include/thfhe_hip.h).
#
# Keeps the reference's names and argument order for the bootstrapped-gate path (3-gen-mk-tfhe/src/gates.jl,
# bootstrap.jl, keyswitch.jl, 3gen_mk_gates.jl, 3gen_mk_internals.jl) so that `using .TFHE_HIP` next to the reference's
# `TFHE` module swaps ONLY that path: keys and ciphertexts are still produced by the reference's own keygen/encrypt, then
# handed over as flat arrays.  Julia is not installed in the build container, so this file is NOT exercised by the test
# suite; the identical call sequence is tested through the Python ctypes layer (torus-fhe_amd/thfhe/__init__.py).
module TFHE_HIP

export HipCloudKey, HipMKCloudKey, gate_nand, gate_or, gate_and, gate_xor, gate_xnor, gate_nor, gate_andny, gate_andyn,
       gate_orny, gate_oryn, gate_mux, gate_not, bootstrap, bootstrap_wo_keyswitch, keyswitch,
       mk_gate_nand_3gen, mk_gate_or_3gen, mk_gate_and_3gen, mk_gate_xor_3gen, mk_gate_3and_3gen, mk_gate_mux_3gen,
       mk_gate_not_3gen, mk_bootstrap_3gen, HipCCSCloudKey, mk_gate_nand, mk_bootstrap, dag_run,
       HipPolyContext, TLweFromLwe, PartialDecrypt, finalDecrypt,
       KmsParams, HipKMSCloudKey, mk_gate_nand_new, mk_bootstrap_new, mk_bootstrap_wo_keyswitch_new, HipPolyMac, poly_mac

const LIB = get(ENV, "THFHE_HIP_LIB", joinpath(@__DIR__, "..", "lib", "libthfhe_hip.so"))

struct Params                      # thfhe_params
    n::Int32; N::Int32; k::Int32; l::Int32; Bgbit::Int32; ks_t::Int32; ks_basebit::Int32; torus_bits::Int32; parties::Int32
end

const NAND, OR, AND, XOR, XNOR, NOR, ANDNY, ANDYN, ORNY, ORYN, MUX, NOT, COPY, AND3 = Int32.(0:13)

lasterror() = unsafe_string(ccall((:thfhe_last_error, LIB), Cstring, ()))
check(rc) = rc == 0 ? nothing : error("libthfhe_hip error $rc: $(lasterror())")

# ---- single key -------------------------------------------------------------------------------------------
mutable struct HipCloudKey
    h::Ptr{Cvoid}
    params::Params
end

"""
    HipCloudKey(params, bk_coeff, ksk; device=0)

`bk_coeff :: Array{Int32}` with memory order [N][k+1][(k+1)l][n] column-major (= C order [n][(k+1)l][k+1][N]):
the coefficient-domain TGSW rows of `BootstrapKey` BEFORE `forward_transform` (bootstrap.jl:11); row index j*l + p.
`ksk :: Array{Int32}` in C order [N][t][base-1][n+1] (`KeyswitchKey.key[h, j, i]` -> a..., b).
"""
function HipCloudKey(p::Params, bk_coeff::Array{Int32}, ksk::Array{Int32}; device::Integer=0)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:thfhe_ctx_create, LIB), Cint, (Ref{Params}, Ptr{Int32}, Ptr{Int32}, Cint, Ref{Ptr{Cvoid}}), p, bk_coeff, ksk, device, h))
    ck = HipCloudKey(h[], p)
    finalizer(c -> ccall((:thfhe_ctx_destroy, LIB), Cvoid, (Ptr{Cvoid},), c.h), ck)
    ck
end

# LWE samples travel as Int32 matrices of size (n+1, count): column g = (a..., b) of gate g
function gates(ck::HipCloudKey, op::Int32, x::Matrix{Int32}, y=nothing, z=nothing)
    out = similar(x)
    yp = y === nothing ? Ptr{Int32}(C_NULL) : pointer(y)
    zp = z === nothing ? Ptr{Int32}(C_NULL) : pointer(z)
    GC.@preserve x y z out check(ccall((:thfhe_gates, LIB), Cint,
        (Ptr{Cvoid}, Cint, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Csize_t), ck.h, op, x, yp, zp, out, size(x, 2)))
    out
end

gate_nand(ck::HipCloudKey, x, y) = gates(ck, NAND, x, y)          # gates.jl:15-18
gate_or(ck::HipCloudKey, x, y) = gates(ck, OR, x, y)              # :27-30
gate_and(ck::HipCloudKey, x, y) = gates(ck, AND, x, y)            # :39-42
gate_xor(ck::HipCloudKey, x, y) = gates(ck, XOR, x, y)            # :51-54
gate_xnor(ck::HipCloudKey, x, y) = gates(ck, XNOR, x, y)          # :63-66
gate_nor(ck::HipCloudKey, x, y) = gates(ck, NOR, x, y)            # :103-106
gate_andny(ck::HipCloudKey, x, y) = gates(ck, ANDNY, x, y)        # :115-118
gate_andyn(ck::HipCloudKey, x, y) = gates(ck, ANDYN, x, y)        # :127-130
gate_orny(ck::HipCloudKey, x, y) = gates(ck, ORNY, x, y)          # :139-142
gate_oryn(ck::HipCloudKey, x, y) = gates(ck, ORYN, x, y)          # :151-154
gate_mux(ck::HipCloudKey, x, y, z) = gates(ck, MUX, x, y, z)      # :163-177
gate_not(ck::HipCloudKey, x) = gates(ck, NOT, x)                  # :76-79

function bootstrap(ck::HipCloudKey, mu::Int32, x::Matrix{Int32})                       # bootstrap.jl:98-101
    out = similar(x)
    check(ccall((:thfhe_bootstrap, LIB), Cint, (Ptr{Cvoid}, Int32, Ptr{Int32}, Ptr{Int32}, Csize_t), ck.h, mu, x, out, size(x, 2)))
    out
end
function bootstrap_wo_keyswitch(ck::HipCloudKey, mu::Int32, x::Matrix{Int32})          # bootstrap.jl:75-88
    out = Matrix{Int32}(undef, ck.params.N + 1, size(x, 2))
    check(ccall((:thfhe_bootstrap_wo_keyswitch, LIB), Cint, (Ptr{Cvoid}, Int32, Ptr{Int32}, Ptr{Int32}, Csize_t), ck.h, mu, x, out, size(x, 2)))
    out
end
function keyswitch(ck::HipCloudKey, u::Matrix{Int32})                                  # keyswitch.jl:45-80
    out = Matrix{Int32}(undef, ck.params.n + 1, size(u, 2))
    check(ccall((:thfhe_keyswitch, LIB), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int32}, Csize_t), ck.h, u, out, size(u, 2)))
    out
end

# ---- 3-gen multi-key ------------------------------------------------------------------------------------------
mutable struct HipMKCloudKey
    h::Ptr{Cvoid}
    params::Params
end

"""
    HipMKCloudKey(params, bk_coeff, ksk; device=0)

`bk_coeff :: Array{Int64}` in C order [P][n][4][l][N]: part_1..part_4 of every `TGswSample_3gen` of every party's
`BootstrapKeyPart_3gen.gsw_key` (coefficient domain, i.e. before `TransformedBootstrapKeyPart_3gen`);
`ksk :: Array{Int32}` in C order [P][N][t][base-1][n+1].  MK samples are Int32 matrices (P*n+1, count): a[:,p] stacked, then b.
"""
function HipMKCloudKey(p::Params, bk_coeff::Array{Int64}, ksk::Array{Int32}; device::Integer=0)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:thfhe_mk_ctx_create, LIB), Cint, (Ref{Params}, Ptr{Int64}, Ptr{Int32}, Cint, Ref{Ptr{Cvoid}}), p, bk_coeff, ksk, device, h))
    ck = HipMKCloudKey(h[], p)
    finalizer(c -> ccall((:thfhe_mk_ctx_destroy, LIB), Cvoid, (Ptr{Cvoid},), c.h), ck)
    ck
end

function mk_gates(ck::HipMKCloudKey, op::Int32, x::Matrix{Int32}, y=nothing, z=nothing)
    out = similar(x)
    yp = y === nothing ? Ptr{Int32}(C_NULL) : pointer(y)
    zp = z === nothing ? Ptr{Int32}(C_NULL) : pointer(z)
    GC.@preserve x y z out check(ccall((:thfhe_mk_gates, LIB), Cint,
        (Ptr{Cvoid}, Cint, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Csize_t), ck.h, op, x, yp, zp, out, size(x, 2)))
    out
end

# the reference passes (bk, ks, x, y); here the context holds both key tables        3gen_mk_gates.jl:8-150
mk_gate_nand_3gen(ck::HipMKCloudKey, x, y) = mk_gates(ck, NAND, x, y)
mk_gate_or_3gen(ck::HipMKCloudKey, x, y) = mk_gates(ck, OR, x, y)
mk_gate_and_3gen(ck::HipMKCloudKey, x, y) = mk_gates(ck, AND, x, y)
mk_gate_xor_3gen(ck::HipMKCloudKey, x, y) = mk_gates(ck, XOR, x, y)
mk_gate_3and_3gen(ck::HipMKCloudKey, x, y, z) = mk_gates(ck, AND3, x, y, z)
mk_gate_mux_3gen(ck::HipMKCloudKey, x, y, z) = mk_gates(ck, MUX, x, y, z)
mk_gate_not_3gen(ck::HipMKCloudKey, x) = mk_gates(ck, NOT, x)

function mk_bootstrap_3gen(ck::HipMKCloudKey, mu::Int64, x::Matrix{Int32})              # 3gen_mk_internals.jl:112-116
    out = similar(x)
    check(ccall((:thfhe_mk_bootstrap, LIB), Cint, (Ptr{Cvoid}, Int64, Ptr{Int32}, Ptr{Int32}, Csize_t), ck.h, mu, x, out, size(x, 2)))
    out
end

# ---- CCS multi-key scheme: mk_gate_nand / mk_bootstrap (mk_gates.jl:7-13, mk_internals.jl:855-858) ---------------------
mutable struct HipCCSCloudKey
    h::Ptr{Cvoid}
    params::Params
end

"""
    HipCCSCloudKey(params, bk, pk, crs, ksk; device=0)

C-order tables: `bk` Int32[P][n][3][l][N] = (d1, f0, f1) of every `MKTGswUESample` of `BootstrapKeyPart.key_uni_enc`;
`pk` Int32[P][l][N] = `PublicKey.b`; `crs` Int32[l][N] = `SharedKey.a`; `ksk` Int32[P][N][t][base-1][n+1].
"""
function HipCCSCloudKey(p::Params, bk::Array{Int32}, pk::Array{Int32}, crs::Array{Int32}, ksk::Array{Int32}; device::Integer=0)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:thfhe_ccs_ctx_create, LIB), Cint, (Ref{Params}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Cint, Ref{Ptr{Cvoid}}),
                p, bk, pk, crs, ksk, device, h))
    ck = HipCCSCloudKey(h[], p)
    finalizer(c -> ccall((:thfhe_ccs_ctx_destroy, LIB), Cvoid, (Ptr{Cvoid},), c.h), ck)
    ck
end

function mk_gate_nand(ck::HipCCSCloudKey, x::Matrix{Int32}, y::Matrix{Int32})
    out = similar(x)
    check(ccall((:thfhe_ccs_gates, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Csize_t), ck.h, NAND, x, y, out, size(x, 2)))
    out
end

function mk_bootstrap(ck::HipCCSCloudKey, mu::Int32, x::Matrix{Int32})
    out = similar(x)
    check(ccall((:thfhe_ccs_bootstrap, LIB), Cint, (Ptr{Cvoid}, Int32, Ptr{Int32}, Ptr{Int32}, Csize_t), ck.h, mu, x, out, size(x, 2)))
    out
end

# ---- gate DAGs: native ASAP scheduler + device-resident executor (thfhe_dag_run) ----------------------------------------
"""
    dag_run(ck, inputs, gates) -> wires

`inputs :: Matrix{Int32}` (n+1, n_inputs); `gates :: Matrix{Int32}` (4, n_gates) = (opcode, in0, in1, in2) per column, 0-based wire
ids, topological order.  Returns the whole wire table (n+1, n_inputs + n_gates).
"""
function dag_run(ck::HipCloudKey, inputs::Matrix{Int32}, gates::Matrix{Int32})
    ni, ng = size(inputs, 2), size(gates, 2)
    wires = zeros(Int32, size(inputs, 1), ni + ng)
    wires[:, 1:ni] .= inputs
    check(ccall((:thfhe_dag_run, LIB), Cint, (Ptr{Cvoid}, Ptr{Int32}, Csize_t, Ptr{Int32}, Csize_t, Ptr{Int64}), ck.h, wires, ni, gates, ng, C_NULL))
    wires
end

"""
    dag_run_batch(ck, inputs, gates[, out_wires]) -> outputs

The reference's loop over test records around one circuit (`for i < test_row_size`, src/KNN_medical_data.cpp:676-691) as ONE evaluation:
`inputs :: Array{Int32,3}` (n+1, n_inputs, instances); every instance walks the levels of `gates` side by side (a level's launch holds
instances x its gates).  `out_wires` (0-based wire ids) selects the wires to return; default: every gate wire.  Returns
(n+1, length(out_wires) or n_gates, instances).
"""
function dag_run_batch(ck::HipCloudKey, inputs::Array{Int32,3}, gates::Matrix{Int32}, out_wires::Union{Nothing, Vector{Int32}}=nothing)
    ni, q, ng = size(inputs, 2), size(inputs, 3), size(gates, 2)
    nout = out_wires === nothing ? ng : length(out_wires)
    out = zeros(Int32, size(inputs, 1), nout, q)
    sel = out_wires === nothing ? Ptr{Int32}(C_NULL) : pointer(out_wires)
    GC.@preserve out_wires check(ccall((:thfhe_dag_run_batch, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Int32}, Csize_t, Ptr{Int32}, Csize_t, Csize_t, Ptr{Int32}, Csize_t, Ptr{Int32}, Ptr{Int64}),
        ck.h, inputs, ni, gates, ng, q, sel, out_wires === nothing ? 0 : nout, out, C_NULL))
    out
end

# thfhe_dag_run_lhe_batch (leveled nodes on TGSW-encrypted bits, include/thfhe_hip.h): the raw binding, arguments as the C prototype
dag_run_lhe_batch_raw(a...) = ccall((:thfhe_dag_run_lhe_batch, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int32}, Csize_t, Ptr{Int32}, Csize_t, Ptr{Cvoid}, Cint, Ptr{Int32}, Cint, Ptr{Int32}, Ptr{Int32}, Cint, Ptr{Cvoid}, Cint, Ptr{Int32}, Cint, Ptr{Cvoid}, Cint, Ptr{Int32}, Cint, Ptr{Int32}, Csize_t, Ptr{Cvoid}, Csize_t, Ptr{Int32}, Csize_t, Ptr{Int32}, Ptr{Int64}), a...)

# ---- after the gate path: TLweFromLwe / PartialDecrypt / finalDecrypt (src/libthfhe.cpp:270-348) ---------------------------
mutable struct HipPolyContext
    h::Ptr{Cvoid}
end
function HipPolyContext(; device::Integer=0, N::Integer=1024)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:thfhe_poly_ctx_create, LIB), Cint, (Cint, Cint, Ref{Ptr{Cvoid}}), device, N, h))
    c = HipPolyContext(h[])
    finalizer(x -> ccall((:thfhe_poly_ctx_destroy, LIB), Cvoid, (Ptr{Cvoid},), x.h), c)
    c
end
function TLweFromLwe(c::HipPolyContext, lwe::Matrix{Int32})                      # (N+1, count) -> a, b of size (N, count)
    cnt = size(lwe, 2); N = size(lwe, 1) - 1
    a, b = zeros(Int32, N, cnt), zeros(Int32, N, cnt)
    check(ccall((:thfhe_tlwe_from_lwe, LIB), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Csize_t), c.h, lwe, a, b, cnt))
    a, b
end
function PartialDecrypt(c::HipPolyContext, key_share::Vector{Int32}, a::Matrix{Int32}, noise::Union{Nothing, Matrix{Int32}}=nothing)
    out = similar(a)
    np = noise === nothing ? Ptr{Int32}(C_NULL) : pointer(noise)
    GC.@preserve noise check(ccall((:thfhe_partial_decrypt, LIB), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Csize_t),
                                   c.h, key_share, a, np, out, size(a, 2)))
    out
end
function finalDecrypt(c::HipPolyContext, b::Matrix{Int32}, partials::Array{Int32, 3})      # partials (N, count, t)
    bits = zeros(Int32, size(b, 2))
    check(ccall((:thfhe_final_decrypt, LIB), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int32}, Cint, Ptr{Int32}, Ptr{Int32}, Csize_t),
                c.h, b, partials, size(partials, 3), C_NULL, bits, size(b, 2)))
    bits .> 0
end

# ---- KMS multi-key scheme (new_mk_gates.jl:1-7, new_mk_internals.jl:302-325) -----------------------------------------------------------
struct KmsParams                   # thfhe_kms_params
    n::Int32; N::Int32; parties::Int32
    l_gsw::Int32; bg_gsw::Int32
    l_lev::Int32; bg_lev::Int32
    l_uni::Int32; bg_uni::Int32
    ks_t::Int32; ks_basebit::Int32
end
mutable struct HipKMSCloudKey      # MKCloudKey_new (mk_api.jl:440-455) on the device
    h::Ptr{Cvoid}
    p::KmsParams
end
# gsw Int64[N, 2, 2 l_gsw, n, P] (TGswSample rows before the forward transform), uni Int64[N, l_uni, 3, P] (d, f0, f1), pk Int64[N, l_uni, P],
# crs Int64[N, l_uni], ksk Int32[n+1, base-1, t, N, P] -- Julia's column-major order of these shapes is the C order the ABI expects
function HipKMSCloudKey(p::KmsParams, gsw::Array{Int64}, uni::Array{Int64}, pk::Array{Int64}, crs::Array{Int64}, ksk::Array{Int32}; device::Integer=0)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:thfhe_kms_ctx_create, LIB), Cint, (Ref{KmsParams}, Ptr{Int64}, Ptr{Int32}, Cint, Ref{Ptr{Cvoid}}), p, gsw, ksk, device, h))
    ck = HipKMSCloudKey(h[], p)
    finalizer(c -> ccall((:thfhe_kms_ctx_destroy, LIB), Cvoid, (Ptr{Cvoid},), c.h), ck)
    check(ccall((:thfhe_kms_set_relin_keys, LIB), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}), ck.h, uni, pk, crs))
    ck
end
# x, y: (P n + 1, count) columns (vec(sample.a); sample.b)
function mk_gate_nand_new(ck::HipKMSCloudKey, x::Matrix{Int32}, y::Matrix{Int32}, fast_boot::Bool=false)      # new_mk_gates.jl:1-7
    out = similar(x)
    check(ccall((:thfhe_kms_gates, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Csize_t, Cint), ck.h, NAND, x, y, out, size(x, 2), fast_boot))
    out
end
function mk_bootstrap_new(ck::HipKMSCloudKey, mu::Int64, x::Matrix{Int32}, fast_boot::Bool=false)               # new_mk_internals.jl:315-325
    out = similar(x)
    check(ccall((:thfhe_kms_bootstrap, LIB), Cint, (Ptr{Cvoid}, Int64, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Csize_t, Cint), ck.h, mu, x, C_NULL, out, size(x, 2), fast_boot))
    out
end
function mk_bootstrap_wo_keyswitch_new(ck::HipKMSCloudKey, mu::Int64, x::Matrix{Int32}, fast_boot::Bool=false)  # new_mk_internals.jl:302-313
    u = Matrix{Int32}(undef, ck.p.parties * ck.p.N + 1, size(x, 2))
    check(ccall((:thfhe_kms_bootstrap, LIB), Cint, (Ptr{Cvoid}, Int64, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Csize_t, Cint), ck.h, mu, x, u, C_NULL, size(x, 2), fast_boot))
    u
end

# ---- exact small x torus polynomial multiply-accumulate (the products of multi-key key generation, multikey_3gen.jl:15-30) ------------
mutable struct HipPolyMac
    h::Ptr{Cvoid}
    N::Int
    bits::Int
end
function HipPolyMac(N::Integer, torus_bits::Integer; device::Integer=0)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:thfhe_pm_ctx_create, LIB), Cint, (Cint, Cint, Cint, Ref{Ptr{Cvoid}}), device, N, torus_bits, h))
    c = HipPolyMac(h[], N, torus_bits)
    finalizer(x -> ccall((:thfhe_pm_ctx_destroy, LIB), Cvoid, (Ptr{Cvoid},), x.h), c)
    c
end
# out[:, j] = addend[:, j] + sum over the columns (j, s, t, sign) of `terms` (0-based, ascending in j) of sign * small[:, s] (*) torus[:, t]
function poly_mac(c::HipPolyMac, small::Matrix{Int32}, torus::Matrix{T}, terms::Matrix{Int32}, n_out::Integer, addend::Union{Nothing, Matrix{T}}=nothing) where {T<:Union{Int32, Int64}}
    out = Matrix{T}(undef, c.N, n_out)
    GC.@preserve addend check(ccall((:thfhe_pm_mac, LIB), Cint, (Ptr{Cvoid}, Ptr{Int32}, Csize_t, Ptr{Cvoid}, Csize_t, Ptr{Int32}, Csize_t, Ptr{Cvoid}, Ptr{Cvoid}, Csize_t),
        c.h, small, size(small, 2), torus, size(torus, 2), terms, size(terms, 2), addend === nothing ? C_NULL : pointer(addend), out, n_out))
    out
end

end # module
